"""The yardstick of the tests that train the WHOLE backbone (``set_train_trunk(k)``): any MBConv block of
tests/detector_ref.eager_forward -- the ones without an expand layer, the 5 x 5 and the stride-2 ones among them -- and the stem,
restated from their helpers ``_conv`` / ``_bn``, evaluated in the dtype of what they are given and differentiated by autograd; float64
is the yardstick, float32 the eager evaluation whose own error the bounds are scaled by.  BN runs on its running statistics and there
is no drop-connect.

Three parts: ``block_forward`` / ``stem_forward``; the vector-Jacobian product of one block or of the stem (``block_vjp`` /
``stem_vjp``: forward(x).backward(dy)); and ``method_yardstick``, the detection loss from the first trainable block's stored input with
P4 -- and where the blocks reach it P3 -- taken from the blocks' own outputs, everything behind them from
tests/detector_bifpn_first_ref.py, tests/detector_bifpn_ref.py and tests/detector_train_ref.py with every pool routed by the device's
stored map (the reason is stated in tests/detector_bifpn_ref.py).  ``cut_p4``: the same graph with P4 detached where the first cell
reads it -- what a backward without the P4 join computes; the tests assert that the device differs from it.

``dw_adjoint``: the adjoint of the depthwise conv under TF "same" padding written out as a gather (the kernels' form), which the CPU
test holds against autograd."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import detector_backbone_ref as KR, detector_bifpn_first_ref as FR, detector_bifpn_ref as BR, detector_ref as R, \
    detector_train_ref as TR

PRE = KR.PRE
STEM = "backbone_net.model."


def block_forward(sd, i: int, spec: dict, x):
    """MBConv block i on the NCHW map x: detector_ref.eager_forward's lines for it, with or without the expand layer."""
    p, sw = f"{PRE}{i}.", F.silu
    inp = x
    if spec["e"] != 1:
        x = sw(R._bn(sd, p + "_bn0", R._conv(sd, p + "_expand_conv", x)))
    x = sw(R._bn(sd, p + "_bn1", R._conv(sd, p + "_depthwise_conv", x, spec["k"], spec["s"], x.shape[1])))
    q = F.adaptive_avg_pool2d(x, 1)
    q = R._conv(sd, p + "_se_expand", sw(R._conv(sd, p + "_se_reduce", q)))
    x = torch.sigmoid(q) * x
    x = R._bn(sd, p + "_bn2", R._conv(sd, p + "_project_conv", x))
    return x + inp if spec["skip"] else x


def stem_forward(sd, x):
    """The stem on the NCHW canvas x."""
    return F.silu(R._bn(sd, STEM + "_bn0", R._conv(sd, STEM + "_conv_stem", x, 3, 2)))


def _state(sd, prefixes, dtype):
    """The entries under `prefixes` in `dtype`; the parameters require grad."""
    out = {}
    for k, v in sd.items():
        if k.startswith(prefixes) and not k.endswith("num_batches_tracked"):
            t = v.detach().cpu().to(dtype).clone()
            out[k] = t if k.endswith(("running_mean", "running_var")) else t.requires_grad_(True)
    return out


def block_vjp(sd, i: int, spec: dict, x, dy, dtype):
    """block_forward(x).backward(dy) in `dtype` -> ({parameter: grad}, the gradient of x)."""
    st = _state(sd, (f"{PRE}{i}.",), dtype)
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    block_forward(st, i, spec, x).backward(dy.detach().cpu().to(dtype))
    return {k: v.grad for k, v in st.items() if v.requires_grad}, x.grad


def stem_vjp(sd, x, dy, dtype):
    """stem_forward(x).backward(dy) in `dtype` -> {parameter: grad}."""
    st = _state(sd, (STEM + "_conv_stem.", STEM + "_bn0."), dtype)
    stem_forward(st, x.detach().cpu().to(dtype)).backward(dy.detach().cpu().to(dtype))
    return {k: v.grad for k, v in st.items() if v.requires_grad}


def train_state(sd, blocks, ncells, dtype):
    """The entries of the given blocks, of every BiFPN cell and of the heads in `dtype`; the parameters require grad."""
    return KR.train_state(sd, blocks, ncells, dtype)


def method_yardstick(sd, cc, nc, ncells, blocks, x_in, p34, routes, anchors, gt, offsets, dtype, cut_p4=False, **kw):
    """detection_loss of the heads behind all `ncells` BiFPN cells behind the MBConv blocks `blocks` (consecutive indices ending with
    the last block), run from the first of these blocks' NCHW input x_in in `dtype`.  P3 / P4 are the inputs of the last two stride-2
    blocks: where `blocks` holds the block in front of one, the map is that block's own output, else the stored NCHW one of p34.
    routes[j]: cell j's ``routes`` -> (classification, regression, {parameter: grad}); a parameter the loss does not reach has a zero
    gradient."""
    from stlpose_amd.efficientdet import block_specs
    specs = block_specs(cc)
    s2 = [i for i, b in enumerate(specs) if b["s"] == 2]
    at = {s2[-2]: 0, s2[-1]: 1}   # the block whose input is P3 / P4
    st = train_state(sd, blocks, ncells, dtype)
    p = [t.detach().cpu().to(dtype) for t in p34]
    x = x_in.detach().cpu().to(dtype)
    for i in blocks:
        if i in at and i > blocks[0]:
            p[at[i]] = x.detach() if cut_p4 and at[i] == 1 else x
        x = block_forward(st, i, specs[i], x)
    levels = BR.levels_of(FR.cell0_forward(st, p[0], p[1], x, routes[0]))
    for j in range(1, ncells):
        levels = BR.levels_of(BR.cell_forward(st, j, levels, routes[j]))
    reg, cls = TR.heads_forward(st, cc, nc, levels)
    c, r, _, _ = TR.detection_loss(reg, cls, anchors, gt, offsets, **kw)
    (c + r).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in st.items() if v.requires_grad}
    return c.detach(), r.detach(), grads


def same_pad_before(n: int, k: int, s: int) -> int:
    return max(0, (-(-n // s) - 1) * s - n + k) // 2


def dw_adjoint(dy, w, H: int, W: int, k: int, s: int):
    """The adjoint of the depthwise k x k / s conv under TF "same" padding as a gather: dy [B, C, ceil(H / s), ceil(W / s)], w
    [C, k, k] -> dx [B, C, H, W]; dx[y, x] = sum over the taps (ky, kx) with (y + py - ky) % s == 0 and (x + px - kx) % s == 0 of
    dy[(y + py - ky) / s, (x + px - kx) / s] w[ky, kx], outputs outside the map dropped."""
    B, C, Ho, Wo = dy.shape
    py, px = same_pad_before(H, k, s), same_pad_before(W, k, s)
    dx = dy.new_zeros(B, C, H, W)
    for y in range(H):
        for x in range(W):
            for ky in range(k):
                for kx in range(k):
                    ty, tx = y + py - ky, x + px - kx
                    if ty % s or tx % s or not (0 <= ty // s < Ho and 0 <= tx // s < Wo):
                        continue
                    dx[:, :, y, x] += dy[:, :, ty // s, tx // s] * w[:, ky, kx]
    return dx


def dw_autograd(x, w, dy, k: int, s: int, z=None):
    """fp-exact reference in the dtype given: F.conv2d under explicit TF-same padding (detector_ref._same), differentiated by autograd ->
    (dx, dw [C, k, k]); z: dx times swish'(z), written as d silu(z) / dz."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    F.conv2d(R._same(x, k, s), w[:, None], None, s, 0, 1, x.shape[1]).backward(dy)
    dx = x.grad
    if z is not None:
        zz = z.clone().requires_grad_(True)
        F.silu(zz).backward(torch.ones_like(zz))
        dx = dx * zz.grad
    return dx, w.grad


CLASSES = KR.CLASSES + ("stem", "stem_bn")


def tensor_class(name: str) -> str:
    """The class of a trunk parameter in the measured-ratio table (CLASSES)."""
    if name.startswith(STEM + "_conv_stem"):
        return "stem"
    if name.startswith(STEM + "_bn0"):
        return "stem_bn"
    return KR.tensor_class(name)
