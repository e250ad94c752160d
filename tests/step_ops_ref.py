"""The yardsticks of the training step's bookkeeping kernels (tests/test_step_ops_cpu.py, tests/test_step_ops_gpu.py): the fused
optimisers, the BatchNorm running statistics, the weight layouts, the split-K slab sums, the head and the masked MSE, each
restated in plain numpy / torch on the CPU.  Nothing here touches the HIP library.

Every reference takes a dtype: torch.float64 is the yardstick, torch.float32 the eager evaluation whose own error e32 scales
the bounds (tests/vgg_layers_ref.py: e <= max(MARGIN * e32, 1e-6 * max|Y|), MARGIN = 8).  The inputs of an op are what the
C ABI receives: the optimisers' `hyper` is the device float[8] (lr, beta1, beta2, eps, weight_decay, momentum, nesterov,
gscale), so beta1 is float32(0.9), converted exactly; stl_bn_running_update's momentum is a float in the same way.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pose_ref
from tests.vgg_layers_ref import MARGIN, ROUND, bound, hold, hold16, rel_err  # noqa: F401  (re-exported)

F64, F32 = torch.float64, torch.float32
INT32_MAX = 0x7FFFFFFF
NSHARD = 2   # STL_NSHARD of include/stlpose_hip.h (tests/test_step_ops_gpu.py asserts it)


# ------------------------------------------------------------------------------------------------ optimisers
def hyper(lr=0.0, b1=0.0, b2=0.0, eps=0.0, wd=0.0, mu=0.0, nesterov=0.0, gscale=1.0) -> np.ndarray:
    """The header's layout, in the float32 the kernel reads."""
    return np.array([lr, b1, b2, eps, wd, mu, nesterov, gscale], dtype=np.float32)


# every configuration the GPU test runs: (name, kind, hyper)
ADAM_CONFIGS = [(f"adam wd {wd} gscale {gs}", "adam", hyper(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=wd, gscale=gs))
                for wd in (0.0, 0.1) for gs in (1.0, 0.125)]
SGD_CONFIGS = [(f"sgd mu {mu} nesterov {int(nest)} wd {wd}", "sgd", hyper(lr=1e-2, wd=wd, mu=mu, nesterov=nest, gscale=0.125))
               for mu, nest in ((0.0, 0.0), (0.9, 0.0), (0.9, 1.0)) for wd in (0.0, 0.1)]
OPT_CONFIGS = ADAM_CONFIGS + SGD_CONFIGS
OPT_SIZES = (1, 255, 10007, 4096 * 256 + 257)   # the last: the first n at which adam_kernel's grid-stride loop takes a second trip
OPT_STEPS = 4
# the terms whose loss a test must notice, and the configurations in which each is active
MUTATIONS = ("weight_decay", "bias_correction1", "bias_correction2", "gscale", "nesterov", "first_step_init")


def mutations_of(kind: str, h: np.ndarray):
    out = []
    if h[4] != 0:
        out.append("weight_decay")
    if h[7] != 1:
        out.append("gscale")
    if kind == "adam":
        out += ["bias_correction1", "bias_correction2"]
    else:
        if h[5] != 0:
            out.append("first_step_init")
            if h[6] != 0:
                out.append("nesterov")
    return out


def opt_data(n: int, seed: int = 0):
    """Parameters, the gradients of OPT_STEPS steps (BEFORE gscale: the kernel multiplies), and what the state buffers hold on
    entry: Adam's moments start at zero; the SGD momentum buffer is prefilled with values that a first step must ignore."""
    g = torch.Generator().manual_seed(1000 + seed + n % 997)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 8.0 for _ in range(OPT_STEPS)]   # * gscale 0.125 -> unit scale
    stale = torch.randn(n, generator=g)
    return p, grads, stale


def adam_step(p, g, m, v, h: np.ndarray, t: int, dtype=F64, drop: str | None = None):
    """One torch.optim.Adam step (L2 weight decay, no amsgrad) of step number t (1-based), out of place.  The bias corrections
    are Python floats, as in torch.optim; p, g, m, v are evaluated in `dtype`."""
    lr, b1, b2, eps, wd, gs = (float(h[i]) for i in (0, 1, 2, 3, 4, 7))
    p, g, m, v = (x.to(dtype) for x in (p, g, m, v))
    if drop != "gscale":
        g = g * gs
    if wd != 0 and drop != "weight_decay":
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1 = 1.0 if drop == "bias_correction1" else 1 - b1 ** t
    bc2 = 1.0 if drop == "bias_correction2" else 1 - b2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def sgd_step(p, g, buf, h: np.ndarray, t: int, dtype=F64, drop: str | None = None):
    """One torch.optim.SGD step (dampening 0) of step number t (1-based); at t == 1 the momentum buffer BECOMES the gradient,
    whatever it held.  Without momentum the buffer is returned as it came."""
    lr, wd, mu, nest, gs = (float(h[i]) for i in (0, 4, 5, 6, 7))
    p, g = p.to(dtype), g.to(dtype)
    if drop != "gscale":
        g = g * gs
    if wd != 0 and drop != "weight_decay":
        g = g + wd * p
    if mu != 0:
        buf = g.clone() if (t == 1 and drop != "first_step_init") else mu * buf.to(dtype) + g
        g = g + mu * buf if (nest != 0 and drop != "nesterov") else buf
    return p - lr * g, buf


def opt_run(kind: str, h: np.ndarray, p, grads, stale, dtype=F64, drop: str | None = None):
    """States after each step: a list of (p, m, v) for Adam, (p, buf) for SGD."""
    out = []
    if kind == "adam":
        state = (p.to(dtype), torch.zeros_like(p, dtype=dtype), torch.zeros_like(p, dtype=dtype))
        for t, g in enumerate(grads, 1):
            state = adam_step(state[0], g, state[1], state[2], h, t, dtype, drop)
            out.append(state)
    else:
        state = (p.to(dtype), stale.to(dtype))
        for t, g in enumerate(grads, 1):
            state = sgd_step(state[0], g, state[1], h, t, dtype, drop)
            out.append(state)
    return out


# ------------------------------------------------------------------------------------------------ BatchNorm bookkeeping
BN_CHANNELS = (1, 48, 300)   # 300: more channels than the block has threads
BN_COUNTS = {"3x7x5": (3, 7, 5), "1x1x1": (1, 1, 1)}   # B, H, W: 105 has no float reciprocal; 1: unbiased == biased variance


def bn_data(count: str, seed: int = 0):
    """Per layer the NHWC-flattened data [n, C] in float64 whose sums the kernel receives.  Layer 1 (C = 48) has channel 5 with
    mean / std about 30 and channel 7 constant (s1 / n - mean^2 is pure rounding noise, of either sign)."""
    b, h, w = BN_COUNTS[count]
    n = b * h * w
    g = torch.Generator().manual_seed(77 + seed + n)
    data = []
    for c in BN_CHANNELS:
        x = torch.randn(n, c, generator=g, dtype=F64) * (0.5 + torch.rand(c, generator=g, dtype=F64)) + torch.randn(c, generator=g, dtype=F64)
        if c == 48:
            x[:, 5] = 30.0 + torch.randn(n, generator=g, dtype=F64)
            x[:, 7] = 0.7317
        data.append(x)
    return data


def bn_sums(x: torch.Tensor) -> torch.Tensor:
    """[NSHARD][2][C] float64 sums of one layer, the rows split UNEVENLY between the shards (and nothing in shard 0 when there
    is one row only), so that no single shard holds the layer's sums."""
    n = x.shape[0]
    cut = n // 3
    parts = [x[:cut], x[cut:]]
    return torch.stack([torch.stack([q.sum(0), (q * q).sum(0)]) for q in parts])


def bn_running_ref(x: torch.Tensor, rm, rv, momentum: float):
    """nn.BatchNorm2d's training-mode update of (running_mean, running_var) from data [n, C], in float64 with the exact count."""
    x = x.double()
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)          # two-pass: exactly 0 for a constant channel
    unb = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * rm.double() + momentum * mean, (1 - momentum) * rv.double() + momentum * unb


def bn_running_bound(x: torch.Tensor, new_rm, new_rv, momentum: float):
    """Elementwise |error| allowed for (running_mean, running_var); derivation in tests/test_step_ops_gpu.py."""
    x = x.double()
    n = x.shape[0]
    u = 2.0 ** -24
    mean, s1n = x.mean(0), (x * x).mean(0)
    var = ((x - mean) ** 2).mean(0)
    k = n / (n - 1) if n > 1 else 1.0
    extra = var * n / (n - 1) ** 2 if n > 1 else 0.0
    noise = 2.0 ** -50 * (s1n + mean * mean) * k
    bm = u * new_rm.abs() + momentum * u * mean.abs() + 2.0 ** -50 * mean.abs()
    bv = u * new_rv.abs() + momentum * (u * ((s1n + 2 * mean * mean) * k + extra) + noise)
    return bm, bv


# ------------------------------------------------------------------------------------------------ stl_weight_prep
# Co, Ci, ks, Cip, patch, has a data-gradient layout, and how the entry is placed (see wprep_layout)
WPREP_ENTRIES = [
    dict(Co=36, Ci=36, ks=1),                               # four partial 32 x 32 tiles shared round robin by two blocks
    dict(Co=40, Ci=72, ks=3),                               # tiles of 32 and 8 channels, nine taps
    dict(Co=5, Ci=3, ks=3),                                 # Ci % 4 != 0: generic path; 135 elements: the next src_off is odd
    dict(Co=8, Ci=16, ks=3),                                # src_off % 4 != 0: the tile path's row-walk load
    dict(Co=8, Ci=8, ks=1, misalign_fwd=True),              # fwd_off % 4 != 0: generic path
    dict(Co=12, Ci=20, ks=3, Cip=24),                       # Cip != Ci: generic path, padding columns stay
    dict(Co=64, Ci=3, ks=3, Cip=32, patch=1),               # the stem: [co][tap * 3 + ci] in 32 columns, data-gradient rows 27..31 stay
    dict(Co=16, Ci=8, ks=3, no_bwd=True),                   # no data-gradient layout
]


def wprep_layout(entries=WPREP_ENTRIES):
    """Place the entries: master offsets back to back, kernel layouts in one buffer with a gap of at least 4 elements
    between any two, each on a multiple of 4 unless the entry asks for a misaligned one.  Returns (rows, master length, wk length, blocks); a row has every field of stl_wprep."""
    rows, so, wo, blk = [], 0, 4, 0
    for e in entries:
        co, ci, ks = e["Co"], e["Ci"], e["ks"]
        patch, cip = e.get("patch", 0), e.get("Cip", e["Ci"])
        t = ks * ks
        fwd_n = co * cip if patch else co * t * cip
        bwd_n = cip * co if patch else ci * t * co
        wo = (wo + 3) // 4 * 4 + (1 if e.get("misalign_fwd") else 0)
        fwd = wo
        wo = (wo + fwd_n + 4 + 3) // 4 * 4
        bwd = -1
        if not e.get("no_bwd"):
            bwd = wo
            wo += bwd_n + 4
        rows.append(dict(src_off=so, fwd_off=fwd, bwd_off=bwd, Co=co, Ci=ci, ks=ks, Cip=cip, patch=patch, blk0=blk))
        so += co * ci * t
        blk += -(-co * ci * t // 1024)
    return rows, so, wo, blk


def wprep_ref(master: torch.Tensor, rows, wk_len: int, grad_dtype, fwd_dtype, sentinel: int) -> torch.Tensor:
    """The buffer stl_weight_prep leaves, as integer bit patterns (int32 for fp32 layouts, int16 for 16-bit ones): permute,
    then .to(dtype); everything else holds the sentinel."""
    it = torch.int32 if grad_dtype == F32 else torch.int16
    wk = torch.full((wk_len,), sentinel, dtype=it)
    for r in rows:
        co, ci, ks, cip = r["Co"], r["Ci"], r["ks"], r["Cip"]
        t = ks * ks
        w = master[r["src_off"]:r["src_off"] + co * ci * t].view(co, ci, ks, ks)
        if r["patch"]:
            f = w.permute(0, 2, 3, 1).reshape(co, t * ci)                  # [co][tap * Ci + ci]
            dst = wk[r["fwd_off"]:r["fwd_off"] + co * cip].view(co, cip)
            dst[:, :t * ci] = f.to(fwd_dtype).view(it)
            if r["bwd_off"] >= 0:
                dst = wk[r["bwd_off"]:r["bwd_off"] + cip * co].view(cip, co)
                dst[:t * ci] = f.t().contiguous().to(grad_dtype).view(it)
        else:
            f = w.permute(0, 2, 3, 1).reshape(co, t, ci)                    # [co][tap][ci]
            dst = wk[r["fwd_off"]:r["fwd_off"] + co * t * cip].view(co, t, cip)
            dst[:, :, :ci] = f.contiguous().to(fwd_dtype).view(it)
            if r["bwd_off"] >= 0:
                b = w.permute(1, 2, 3, 0).reshape(ci, t, co).flip(1)        # [ci][flipped tap][co]
                wk[r["bwd_off"]:r["bwd_off"] + ci * t * co] = b.contiguous().to(grad_dtype).view(it).reshape(-1)
    return wk


# ------------------------------------------------------------------------------------------------ stl_reduce_slabs
SLAB_NSPLIT = (1, 3, 4, 7, 8, 9, 13, 21)   # the 8-, 4- and 1-slab loops and their tails
SLAB_ENTRIES = [
    dict(Co=36, Ci=36, ks=1),                               # vector path, two blocks, the second one partial
    dict(Co=40, Ci=72, ks=3, gap=8),                        # vector path with a slab stride above Co * taps * Ci
    dict(Co=5, Ci=3, ks=3, gap=5),                          # scalar path, strided
    dict(Co=64, Ci=3, ks=3, Cip=32, patch=1),               # scalar path, patch entry: [co][32] slabs, 27 columns read
    dict(Co=8, Ci=16, ks=3),                                # vector path again, behind the scalar entries
]
SLAB_SENTINEL = -12345.0


def slab_layout(nsplit: int, entries=SLAB_ENTRIES):
    """Rows with every field of stl_slab, + partial and gradient lengths and the block count.  Gradients lie OIHW with a gap
    of 3 sentinels between entries; partial offsets are multiples of 4."""
    rows, po, go, blk = [], 0, 3, 0
    for e in entries:
        co, ci, ks = e["Co"], e["Ci"], e["ks"]
        patch, cip = e.get("patch", 0), e.get("Cip", e["Ci"])
        t = ks * ks
        slab = co * cip if patch else co * t * ci
        stride = slab + e.get("gap", 0)
        rows.append(dict(part_off=po, grad_off=go, nsplit=nsplit, Co=co, Ci=ci, ks=ks, Cip=cip, patch=patch, blk0=blk,
                         pad=stride if e.get("gap") else 0, slab=slab, stride=stride))
        po += (nsplit * stride + 3) // 4 * 4
        go += co * ci * t + 3
        blk += -(-co * ci * t // 1024)
    return rows, po, go, blk


def slab_partials(rows, total: int, seed: int = 0) -> torch.Tensor:
    """fp32 partial sums with six decades of dynamic range (randn * 10^U(-3, 3)), NaN wherever no slab lies (the strides'
    gaps, and the padding columns 27..31 of a patch slab): none of those may be read."""
    g = torch.Generator().manual_seed(4242 + seed + total)
    buf = torch.full((total,), float("nan"))
    for r in rows:
        for s in range(r["nsplit"]):
            v = torch.randn(r["slab"], generator=g) * 10.0 ** (torch.rand(r["slab"], generator=g) * 6 - 3)
            if r["patch"]:
                v.view(r["Co"], r["Cip"])[:, r["ks"] ** 2 * r["Ci"]:] = float("nan")
            o = r["part_off"] + s * r["stride"]
            buf[o:o + r["slab"]] = v
    return buf


def slab_terms(partials: torch.Tensor, r) -> torch.Tensor:
    """[nsplit, Co, Ci, ks, ks]: the terms of every gradient element, in the gradient's OIHW order."""
    co, ci, ks, cip = r["Co"], r["Ci"], r["ks"], r["Cip"]
    t = ks * ks
    p = torch.stack([partials[r["part_off"] + s * r["stride"]:][:r["slab"]] for s in range(r["nsplit"])])
    if r["patch"]:
        p = p.view(-1, co, cip)[:, :, :t * ci].reshape(-1, co, ks, ks, ci)
    else:
        p = p.view(-1, co, ks, ks, ci)
    return p.permute(0, 1, 4, 2, 3).contiguous()


def sum_in_slab_order(terms: torch.Tensor) -> torch.Tensor:
    """The vector path (Ci % 4 == 0, no patch): from 0, one slab after another, each addition rounded in the terms' dtype."""
    s = torch.zeros_like(terms[0])
    for k in range(terms.shape[0]):
        s = s + terms[k]
    return s


def sum_pairwise_by_eight(terms: torch.Tensor) -> torch.Tensor:
    """The scalar path: full groups of eight slabs are added pairwise, ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)), and
    the group's sum to the running sum; the slabs left over one after another."""
    s = torch.zeros_like(terms[0])
    n, k = terms.shape[0], 0
    while k + 8 <= n:
        a = terms[k:k + 8]
        s = s + (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])))
        k += 8
    while k < n:
        s = s + terms[k]
        k += 1
    return s


def slab_is_vector(r) -> bool:
    return not r["patch"] and r["Ci"] % 4 == 0


def slab_ref(partials: torch.Tensor, rows, grad_len: int, dtype=F32, only=None) -> torch.Tensor:
    """The gradient buffer after stl_reduce_slabs (only = the indices of the rows a range call covers), each row in ITS order
    in `dtype`; every other element holds SLAB_SENTINEL."""
    out = torch.full((grad_len,), SLAB_SENTINEL, dtype=dtype)
    for i, r in enumerate(rows):
        if only is not None and i not in only:
            continue
        terms = slab_terms(partials, r).to(dtype)
        s = sum_in_slab_order(terms) if slab_is_vector(r) else sum_pairwise_by_eight(terms)
        out[r["grad_off"]:r["grad_off"] + s.numel()] = s.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ head
HEAD_J = (16, 17)
HEAD_CI = (16, 32, 48, 64)
HEAD_PIXELS = {"105": (3, 7, 5), "306": (2, 17, 9)}   # B, H, W: less than one 256-pixel chunk; a ragged second chunk
HEAD_NBLK = (1, 3, 5)                                  # 5: more blocks than chunks


def head_data(j: int, ci: int, pixels: str, xdtype, seed: int = 0):
    """x NCHW in the values its storage type holds, w [J, Ci], bias [J], dout [B, J, H, W]."""
    b, h, w = HEAD_PIXELS[pixels]
    g = torch.Generator().manual_seed(j * 1000 + ci * 10 + b + seed)
    x = torch.randn(b, ci, h, w, generator=g).to(xdtype).float()
    wt = torch.randn(j, ci, generator=g) * 0.2
    bias = torch.randn(j, generator=g)
    dout = torch.randn(b, j, h, w, generator=g)
    return x, wt, bias, dout


def head_ref(x, w, bias, dout, dtype=F64):
    """out, dx (NCHW), dw [J, Ci], db [J] of the 1 x 1 conv and its autograd in `dtype`."""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    w4 = w.detach().clone().to(dtype).view(*w.shape, 1, 1).requires_grad_(True)
    b = bias.detach().clone().to(dtype).requires_grad_(True)
    out = F.conv2d(x, w4, b)
    out.backward(dout.to(dtype))
    return out.detach(), x.grad, w4.grad.view(w.shape), b.grad


# ------------------------------------------------------------------------------------------------ loss
def mse_data(b: int, j: int, hw: int, seed: int = 0):
    g = torch.Generator().manual_seed(b * 100 + j * 10 + hw + seed)
    o = torch.randn(b, j, hw, generator=g)
    t = torch.rand(b, j, hw, generator=g)
    tw = torch.rand(b, j, 1, generator=g) + 0.5
    tw[0, 1] = 0.0                      # an invisible joint: its gradient is exactly 0
    tw[b - 1, j - 1] = 1.0
    return o, t, tw


def mse_ref(o, t, tw, gscale: float, dtype=F64):
    """PersonMSELoss (oracle.pose_ref.person_mse_loss) and the gradient of gscale * loss in `dtype`."""
    o = o.detach().clone().to(dtype).requires_grad_(True)
    loss = pose_ref.person_mse_loss(o, t.to(dtype), tw.to(dtype))
    (loss * gscale).backward()
    return loss.detach(), o.grad
