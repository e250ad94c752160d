"""GPU: the kernels that turn a backward pass into a training step (csrc/elementwise.hip), through the C ABI, each against the
fp64 yardstick of tests/step_ops_ref.py: stl_adam_step / stl_sgd_step, stl_bn_running_update / stl_bn_param_grads,
stl_weight_prep, stl_reduce_slabs / stl_reduce_slabs_range, stl_head_forward / stl_head_backward, stl_mse_loss /
stl_sum_partials.  Every output is prefilled with NaN, or with a sentinel where gaps must stay untouched, and every op runs
twice (bit-equal results).

Bounds (tests/vgg_layers_ref.py).  Ops that move, round or sum values in a documented order are held bit for bit:
stl_weight_prep, stl_bn_param_grads, stl_reduce_slabs (both summation orders restated in fp32), every skip rule.  fp32
arithmetic is held to e <= max(8 * e32, 1e-6) relative to max|Y|, e32 the error of torch's fp32 evaluation of the same inputs;
tensors stored in 16 bits elementwise to one rounding of Y more.  stl_bn_running_update has a bound of its own, derived at
its test.

Measured on the MI355X, e / e32 and the largest e per op:
* stl_weight_prep (fp32, bf16, f16, mixed), stl_bn_param_grads, stl_reduce_slabs / stl_reduce_slabs_range against the fp32
  restatement of their orders, every skip rule of the optimisers and of stl_bn_running_update: bit-equal.
* stl_adam_step: p 0.40 - 1.24 (e <= 1.6e-7), m 0.47 - 2.50 (e <= 5.5e-6, at n = 1 where the one element cancels), v 0.75 - 1.00
  (e <= 1.9e-7).  stl_sgd_step: p 0.74 - 1.02 (e <= 1.5e-7), buffer 0.06 - 1.04 (e <= 5.3e-7; e32 = 0 without momentum).
* stl_bn_running_update: largest |error| / allowed 0.90 at n = 105, 0.87 at n = 1 (one fp32 rounding of the result); the running variance
  of the channel with mean / std = 30 at n = 105: |error| 3.5e-6 = 45 roundings
  of the result, 0.21 of the allowance -- the rebuilt count is what the error is made of there; momentum 0: bit-unchanged.
* stl_reduce_slabs against fp64: 0.56 - 1.54, e <= 1.8e-7 (below the floor).
* stl_head_forward: fp32, bf16, f16 ratio 1.00 (e <= 4.8e-7).  stl_head_backward: dx fp32 ratio 1.00 (e <= 1.9e-7), dx bf16 (both
  16-bit forms) largest |error| / allowed 0.995; dw 0.48 - 2.19 (e <= 3.0e-7), db 0.25 - 1.86 (e <= 1.7e-7).
* stl_mse_loss: loss 0.06 - 1.00 (e <= 1.8e-8), the partials summed in fp64 0.01 - 0.40, dout 0.78 - 1.00 (e <= 1.4e-7),
  stl_sum_partials with accumulate 1.00 (e <= 3.3e-8).

Two disagreements these tests found, both settled in the code: bn_running_kernel skipped only the channel with non-finite
sums where include/stlpose_hip.h promises that the LAYER keeps its statistics (now a block-wide vote before any store), and
stl_head_backward refused Ci = 64 (a limit J * Ci + J <= 1024 left from an earlier kernel) although its own next check, the
kernel and the W64 head allow it.  stl_head_forward takes every Ci % 8 == 0 up to 512, so Ci = 24 and 80 are refused by the
backward only; the header says so now.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stlpose_amd import capi
from tests import step_ops_ref as R

pytestmark = pytest.mark.gpu

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
NAN = float("nan")
INT32_MAX = R.INT32_MAX


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def table(cls, rows):
    """A device table of `cls` records from dict rows (keys that are no field of the record are skipped)."""
    tab = (cls * len(rows))()
    names = {f[0] for f in cls._fields_}
    for e, r in zip(tab, rows):
        for k, v in r.items():
            if k in names:
                setattr(e, k, v)
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()


def same_bits(a, b):
    """Bit equality of two tensors of one dtype (NaN payloads and signed zeros included)."""
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it).cpu(), b.contiguous().view(it).cpu())


def test_constants():
    assert capi.NSHARD == R.NSHARD and C.sizeof(capi.Slab) % 4 == 0


# ------------------------------------------------------------------------------------------------ stl_adam_step / stl_sgd_step
def opt_gpu(kind, h, p, grads, state, words=None, step0=0):
    """Run the steps on the GPU.  state: (m, v) or (buf,) on entry; words: per call None (overflow = NULL) or the overflow
    word's value.  Returns the states after each call, (p, m, v) / (p, buf), and what the step word read."""
    hd = torch.from_numpy(h).cuda()
    bufs = [p.clone().cuda()] + [s.clone().cuda() for s in state]
    step = torch.tensor([step0], dtype=torch.int32, device="cuda")
    states, steps = [], []
    for i, g in enumerate(grads):
        gd = g.cuda()
        ov = None if words is None or words[i] is None else torch.tensor([words[i]], dtype=torch.int32, device="cuda")
        capi.call("stl_adam_step" if kind == "adam" else "stl_sgd_step", *(b.data_ptr() for b in bufs[:1]), gd.data_ptr(),
                  *(b.data_ptr() for b in bufs[1:]), p.numel(), hd.data_ptr(), step.data_ptr(), ptr(ov), stream())
        torch.cuda.synchronize()
        states.append(tuple(b.clone() for b in bufs))
        steps.append(int(step.item()))
        if ov is not None:
            assert int(ov.item()) == words[i]   # the optimisers only read the word
    return states, steps


def entry_state(kind, n, stale):
    return (torch.zeros(n), torch.zeros(n)) if kind == "adam" else (stale,)


def assert_same_states(a, b, what=""):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        for x, y in zip(sa, sb):
            assert same_bits(x, y), what


@functools.lru_cache(maxsize=None)
def opt_reference(ci, n):
    _, kind, h = R.OPT_CONFIGS[ci]
    p, grads, stale = R.opt_data(n)
    return R.opt_run(kind, h, p, grads, stale, F64), R.opt_run(kind, h, p, grads, stale, F32)


@pytest.mark.parametrize("n", R.OPT_SIZES)
@pytest.mark.parametrize("ci", range(len(R.OPT_CONFIGS)), ids=[c[0] for c in R.OPT_CONFIGS])
def test_optimisers_are_torch_optim(ci, n):
    name, kind, h = R.OPT_CONFIGS[ci]
    p, grads, stale = R.opt_data(n)
    y64, y32 = opt_reference(ci, n)
    got, steps = opt_gpu(kind, h, p, grads, entry_state(kind, n, stale))
    again, _ = opt_gpu(kind, h, p, grads, entry_state(kind, n, stale))
    assert_same_states(got, again, "two runs differ")
    assert steps == [1, 2, 3, 4]
    for t, (sg, s64, s32) in enumerate(zip(got, y64, y32), 1):
        for what, xg, x64, x32 in zip(("p", "m", "v") if kind == "adam" else ("p", "buf"), sg, s64, s32):
            R.hold(f"{'stl_adam_step' if kind == 'adam' else 'stl_sgd_step'} {name} n {n} step {t} {what}", xg.cpu(), x64, x32)
    if kind == "sgd" and h[5] == 0:
        assert same_bits(got[-1][1].cpu(), stale)   # no momentum: the buffer is not touched


SKIP_CONFIGS = [("adam", R.hyper(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, gscale=4.0)),
                ("sgd", R.hyper(lr=1e-2, wd=0.1, mu=0.9, nesterov=1.0, gscale=4.0))]


def skip_data(kind, n=10007, fresh=False):
    """fresh: the state of a run that starts (zero moments; a NaN momentum buffer, which a first step must not read); else a
    state in use, so that "unchanged" says something."""
    p, grads, stale = R.opt_data(n, seed=5)
    grads = [g / 32 for g in grads]   # * gscale 4 -> unit scale
    g = torch.Generator().manual_seed(11)
    if fresh:
        state = (torch.zeros(n), torch.zeros(n)) if kind == "adam" else (torch.full((n,), NAN),)
    else:
        state = (torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01) if kind == "adam" else (stale,)
    return p, grads, state


@pytest.mark.parametrize("kind,h", SKIP_CONFIGS, ids=["adam", "sgd"])
def test_optimisers_keep_elements_with_a_non_finite_gradient(kind, h):
    p, grads, state = skip_data(kind)
    n = p.numel()
    bad = {0: NAN, 255: float("inf"), 256: float("-inf"), n - 1: 1e38}   # 1e38 * gscale 4 overflows fp32
    assert 1e38 < 3.4e38 < 1e38 * float(h[7])
    idx = torch.tensor(list(bad))
    dirty = []
    for g in grads:
        d = g.clone()
        d[idx] = torch.tensor(list(bad.values()))
        dirty.append(d)
    step0 = 1 if kind == "sgd" else 0   # SGD: the prefilled buffer is in use, so that "unchanged" says something
    clean, _ = opt_gpu(kind, h, p, grads, state, step0=step0)
    got, steps = opt_gpu(kind, h, p, dirty, state, step0=step0)
    assert steps == [step0 + t for t in (1, 2, 3, 4)]   # the step itself counts
    keep = torch.ones(n, dtype=torch.bool)
    keep[idx] = False
    for sg, sc in zip(got, clean):
        for xg, xc, x0 in zip(sg, sc, (p,) + tuple(state)):
            assert same_bits(xg.cpu()[idx], x0[idx])           # weight and moments as they were
            assert same_bits(xg.cpu()[keep], xc.cpu()[keep])   # every other element as without them
            assert not same_bits(xc.cpu()[idx], x0[idx])


@pytest.mark.parametrize("kind,h", SKIP_CONFIGS, ids=["adam", "sgd"])
def test_a_skipped_step_is_not_counted(kind, h):
    p, grads, state = skip_data(kind, fresh=True)
    got, steps = opt_gpu(kind, h, p, grads, state, words=[INT32_MAX, 1, 0, INT32_MAX])   # armed, set, set, armed
    assert steps == [1, -2, -2, 2]
    for k in (1, 2):   # the skipped calls change no bit
        for x, y in zip(got[k], got[0]):
            assert same_bits(x, y)
    two, steps2 = opt_gpu(kind, h, p, [grads[0], grads[3]], state, words=[None, None])   # overflow = NULL behaves as armed
    assert steps2 == [1, 2]
    assert_same_states([got[0], got[3]], two)
    # the fourth call is the reference's SECOND step (bias corrections with t = 2; SGD: the buffer of step 1 is in use)
    y64, y32 = (R.opt_run(kind, h, p, [grads[0], grads[3]], state[-1], dt) for dt in (F64, F32))
    for what, xg, x64, x32 in zip(("p", "m", "v") if kind == "adam" else ("p", "buf"), got[3], y64[1], y32[1]):
        R.hold(f"stl_{kind}_step after two skipped calls {what}", xg.cpu(), x64, x32)
    if kind == "adam":   # had the skipped calls been counted, the bias corrections would be those of t = 4
        wrong = R.adam_step(y64[0][0], grads[3], y64[0][1], y64[0][2], h, 4)
        assert R.rel_err(got[3][0].cpu(), wrong[0]) > 100 * R.bound(R.rel_err(y32[1][0], y64[1][0]))


def test_sgd_first_call_skipped_then_first_step_and_resume():
    kind, h = SKIP_CONFIGS[1]
    p, grads, nanbuf = skip_data(kind, fresh=True)
    got, steps = opt_gpu(kind, h, p, grads[:3], nanbuf, words=[7, INT32_MAX, INT32_MAX])
    assert steps == [-1, 1, 2]
    assert same_bits(got[0][0].cpu(), p) and same_bits(got[0][1].cpu(), nanbuf[0])
    plain, _ = opt_gpu(kind, h, p, grads[1:3], nanbuf)
    assert_same_states(got[1:], plain)                       # the next call is a first step: the buffer becomes g
    y64, y32 = (R.opt_run(kind, h, p, grads[1:3], nanbuf[0], dt) for dt in (F64, F32))
    for t in (0, 1):
        for what, xg, x64, x32 in zip(("p", "buf"), got[1 + t], y64[t], y32[t]):
            R.hold(f"stl_sgd_step first call skipped, step {t + 1} {what}", xg.cpu(), x64, x32)
    # resume: step >= 1 on entry, the prefilled buffer is used
    _, _, stale = R.opt_data(p.numel(), seed=5)
    res, steps = opt_gpu(kind, h, p, grads[:1], (stale,), step0=1)
    assert steps == [2]
    for what, xg, x64, x32 in zip(("p", "buf"), res[0], R.sgd_step(p, grads[0], stale, h, 2, F64), R.sgd_step(p, grads[0], stale, h, 2, F32)):
        R.hold(f"stl_sgd_step resumed {what}", xg.cpu(), x64, x32)
    fresh = R.sgd_step(p, grads[0], stale, h, 1, F64)
    assert R.rel_err(res[0][1].cpu(), fresh[1]) > 0.1        # a first step would have dropped the buffer


# ------------------------------------------------------------------------------------------------ stl_bn_running_update / stl_bn_param_grads
# The bound of stl_bn_running_update.  The kernel forms everything in fp64 from the fp64 sums and rounds each result once to
# fp32: |Y| * 2**-24.  Its count is rebuilt from a float: n' = 1 / (double)(float)(1 / n) = n (1 + d) with |d| <= 2**-24 =: u (one
# float rounding of 1 / n).  Then mean' = s0 / n' = mean (1 - d): |error| <= u |mean|.  var' = s1 / n' - mean'^2
# = (s1 / n)(1 - d) - mean^2 (1 - 2 d): |error| <= u (|s1 / n| + 2 mean^2).  The unbiased factor n' / (n' - 1) = n / (n - 1) *
# (1 - d / (n - 1)) scales that error by n / (n - 1) and adds u var n / (n - 1)^2.  Both enter the buffers times the momentum.  fp64's
# own rounding in s1 / n - mean^2 (cancellation) is 2**-50 (s1 / n + mean^2) at the most.  R.bn_running_bound adds these up.
SENT = -7.75   # in the gaps of the buffer and gradient arenas


def bn_arena(count, with_stats=True):
    """Three layers: the table rows, the stats arena (NaN between the layers' blocks), data, and arena lengths."""
    data = R.bn_data(count)
    rows, so, po, bo = [], 3, 5, 2
    for x in data:
        c = x.shape[1]
        rows.append(dict(stats_off=so, param_off=po, buf_off=bo, C=c, inv_count=float(np.float32(1.0 / x.shape[0]))))
        so += R.NSHARD * 2 * c + 3
        po += 2 * c + 7
        bo += 2 * c + 5
    stats = torch.full((so,), NAN, dtype=F64)
    for r, x in zip(rows, data):
        stats[r["stats_off"]:r["stats_off"] + R.NSHARD * 2 * r["C"]] = R.bn_sums(x).reshape(-1)
    return rows, stats, data, po, bo


def bn_buffers(rows, nbuf):
    g = torch.Generator().manual_seed(99)
    buf = torch.full((nbuf,), SENT)
    for r in rows:
        c = r["C"]
        buf[r["buf_off"]:r["buf_off"] + c] = torch.randn(c, generator=g)
        buf[r["buf_off"] + c:r["buf_off"] + 2 * c] = torch.rand(c, generator=g) + 0.5
    return buf


def bn_run(rows, stats, buf, momentum, nbt, word):
    tab = table(capi.BNRec, rows)
    sd, bd = stats.cuda(), buf.clone().cuda()
    nd = None if nbt is None else nbt.clone().cuda()
    wd = None if word is None else torch.tensor([word], dtype=torch.int32, device="cuda")
    capi.call("stl_bn_running_update", sd.data_ptr(), bd.data_ptr(), ptr(nd), tab.data_ptr(), len(rows), momentum, ptr(wd), stream())
    torch.cuda.synchronize()
    return bd.cpu(), None if nd is None else nd.cpu(), None if wd is None else int(wd.item())


@pytest.mark.parametrize("with_nbt", [True, False], ids=["nbt", "no_nbt"])
@pytest.mark.parametrize("momentum", [0.1, 0.0])
@pytest.mark.parametrize("count", list(R.BN_COUNTS))
def test_bn_running_update_is_batchnorm2d(count, momentum, with_nbt):
    rows, stats, data, _, nbuf = bn_arena(count)
    buf = bn_buffers(rows, nbuf)
    nbt = torch.tensor([5, 0, 41], dtype=torch.int64) if with_nbt else None
    mom = float(np.float32(momentum))
    got, n1, word = bn_run(rows, stats, buf, momentum, nbt, INT32_MAX)
    again, _, _ = bn_run(rows, stats, buf, momentum, nbt, None)
    assert same_bits(got, again) and word == INT32_MAX   # finite sums: the word stays armed; NULL is the same update
    if with_nbt:
        assert n1.tolist() == [6, 1, 42]                 # once per layer
    mask = torch.zeros(nbuf, dtype=torch.bool)
    worst = 0.0
    for r, x in zip(rows, data):
        c, o = r["C"], r["buf_off"]
        mask[o:o + 2 * c] = True
        rm, rv = buf[o:o + c], buf[o + c:o + 2 * c]
        if momentum == 0.0:
            assert same_bits(got[o:o + 2 * c], buf[o:o + 2 * c])
            continue
        ym, yv = R.bn_running_ref(x, rm, rv, mom)
        bm, bv = R.bn_running_bound(x, ym, yv, mom)
        em, ev = (got[o:o + c].double() - ym).abs(), (got[o + c:o + 2 * c].double() - yv).abs()
        worst = max(worst, (em / bm).max().item(), (ev / bv).max().item())
        assert (em <= bm).all() and (ev <= bv).all(), (c, (em / bm).max().item(), (ev / bv).max().item())
        assert (got[o + c:o + 2 * c] >= 0).all()
        if c == 48:
            print(f"stl_bn_running_update count {count}: running_var of the mean / std = 30 channel: |error| {ev[5].item():.2e} = "
                  f"{ev[5].item() / (2.0 ** -24 * yv[5].abs().item()):.1f} roundings of the result, {(ev[5] / bv[5]).item():.3f} of the allowance")
            # the constant channel: variance 0 after the clamp, so exactly (1 - momentum) * old
            assert got[o + c + 7].item() == np.float32((1.0 - mom) * float(rv[7])) and got[o + c + 7].item() > 0
    print(f"stl_bn_running_update count {count} momentum {momentum}: largest |error| / allowed {worst:.3f}")
    assert (got[~mask] == SENT).all()


def test_bn_running_update_keeps_a_layer_with_non_finite_sums():
    rows, stats, data, _, nbuf = bn_arena("3x7x5")
    buf = bn_buffers(rows, nbuf)
    nbt = torch.tensor([5, 0, 41], dtype=torch.int64)
    clean, _, _ = bn_run(rows, stats, buf, 0.1, nbt, INT32_MAX)
    dirty = stats.clone()
    r1, r2 = rows[1], rows[2]
    dirty[r1["stats_off"] + 2 * r1["C"] + 11] = float("inf")             # layer 1: s0 of channel 11, in shard 1
    dirty[r2["stats_off"] + r2["C"] + 280] = NAN                          # layer 2: s1 of channel 280 (a thread's second channel), shard 0
    got, n1, word = bn_run(rows, dirty, buf, 0.1, nbt, INT32_MAX)
    again, _, word2 = bn_run(rows, dirty, buf, 0.1, nbt, INT32_MAX)
    assert same_bits(got, again) and word == word2 == 1                   # the first such layer
    assert n1.tolist() == [6, 1, 42]                                      # one forward pass, counted
    o, c = rows[0]["buf_off"], rows[0]["C"]
    assert same_bits(got[o:o + 2 * c], clean[o:o + 2 * c]) and not same_bits(got[o:o + 2 * c], buf[o:o + 2 * c])   # layer 0 is updated
    assert same_bits(got[o + 2 * c:], buf[o + 2 * c:])                    # EVERY channel of layers 1 and 2, and the gaps, as they were
    _, _, none = bn_run(rows, dirty, buf, 0.1, None, None)                # overflow = NULL, nbt = NULL: nothing to report to
    assert none is None
    _, _, low = bn_run(rows, dirty, buf, 0.1, None, 0)                    # an earlier report stays (atomic min)
    assert low == 0


def test_bn_param_grads_are_the_rounded_shard_sums():
    rows, _, _, ngrad, _ = bn_arena("3x7x5")
    g = torch.Generator().manual_seed(31)
    nst = rows[-1]["stats_off"] + R.NSHARD * 2 * rows[-1]["C"] + 3
    rst = torch.full((nst,), NAN, dtype=F64)
    exp = torch.full((ngrad,), SENT)
    for r in rows:
        c = r["C"]
        blk = torch.randn(R.NSHARD, 2, c, generator=g, dtype=F64) * 10.0 ** (torch.rand(R.NSHARD, 2, c, generator=g, dtype=F64) * 4 - 2)
        rst[r["stats_off"]:r["stats_off"] + blk.numel()] = blk.reshape(-1)
        s = torch.zeros(2, c, dtype=F64)
        for k in range(R.NSHARD):
            s = s + blk[k]
        exp[r["param_off"]:r["param_off"] + c] = s[1].float()            # dgamma = r2
        exp[r["param_off"] + c:r["param_off"] + 2 * c] = s[0].float()    # dbeta = r1
    tab, rd = table(capi.BNRec, rows), rst.cuda()

    def run():
        grads = torch.full((ngrad,), SENT, device="cuda")
        capi.call("stl_bn_param_grads", rd.data_ptr(), grads.data_ptr(), tab.data_ptr(), len(rows), stream())
        torch.cuda.synchronize()
        return grads
    a, b = run(), run()
    assert same_bits(a, b) and same_bits(a.cpu(), exp)


# ------------------------------------------------------------------------------------------------ stl_weight_prep
WPREP_DT = {"fp32": (capi.F32, F32, F32), "bf16": (capi.BF16, BF16, BF16), "f16": (capi.F16, F16, F16),
            "mixed": (capi.dt2(capi.BF16, capi.F16), BF16, F16)}   # code, data-gradient layouts, forward layouts


@pytest.mark.parametrize("dt", list(WPREP_DT))
def test_weight_prep_is_permute_and_round(dt):
    code, gd, fd = WPREP_DT[dt]
    rows, nsrc, nwk, nblk = R.wprep_layout()
    master = torch.randn(nsrc, generator=torch.Generator().manual_seed(3))
    sent = 0x5A5A5A5A if gd == F32 else 0x5A5A
    exp = R.wprep_ref(master, rows, nwk, gd, fd, sent)
    md, tab = master.cuda(), table(capi.WPrep, rows)
    assert md.data_ptr() % 16 == 0

    def run():
        wk = torch.full((nwk,), sent, dtype=exp.dtype, device="cuda")
        capi.call("stl_weight_prep", code, md.data_ptr(), wk.data_ptr(), tab.data_ptr(), len(rows), nblk, stream())
        torch.cuda.synchronize()
        return wk
    a, b = run(), run()
    assert torch.equal(a, b)
    a = a.cpu()
    for i, r in enumerate(rows):   # per layout first, for a readable failure
        t = r["ks"] ** 2
        nf = r["Co"] * (r["Cip"] if r["patch"] else t * r["Cip"])
        assert torch.equal(a[r["fwd_off"]:r["fwd_off"] + nf], exp[r["fwd_off"]:r["fwd_off"] + nf]), f"entry {i}: forward layout"
        if r["bwd_off"] >= 0:
            nb = r["Cip"] * r["Co"] if r["patch"] else r["Ci"] * t * r["Co"]
            assert torch.equal(a[r["bwd_off"]:r["bwd_off"] + nb], exp[r["bwd_off"]:r["bwd_off"] + nb]), f"entry {i}: data-gradient layout"
    assert torch.equal(a, exp)     # and everything outside the layouts holds the sentinel


# ------------------------------------------------------------------------------------------------ stl_reduce_slabs / stl_reduce_slabs_range
@pytest.mark.parametrize("nsplit", R.SLAB_NSPLIT)
def test_reduce_slabs_sums_in_its_documented_orders(nsplit):
    rows, npart, ngrad, nblk = R.slab_layout(nsplit)
    partials = R.slab_partials(rows, npart)
    exp = R.slab_ref(partials, rows, ngrad, F32)
    pd, tab = partials.cuda(), table(capi.Slab, rows)
    assert pd.data_ptr() % 16 == 0

    def full():
        grads = torch.full((ngrad,), R.SLAB_SENTINEL, device="cuda")
        capi.call("stl_reduce_slabs", pd.data_ptr(), grads.data_ptr(), tab.data_ptr(), len(rows), nblk, stream())
        torch.cuda.synchronize()
        return grads
    a, b = full(), full()
    assert same_bits(a, b)
    a = a.cpu()
    for i, r in enumerate(rows):
        n = r["Co"] * r["Ci"] * r["ks"] ** 2
        sl = slice(r["grad_off"], r["grad_off"] + n)
        assert not torch.isnan(a[sl]).any(), f"entry {i}: a gap was read"
        assert same_bits(a[sl], exp[sl]), f"entry {i} ({'vector' if R.slab_is_vector(r) else 'scalar'} path)"
        terms = R.slab_terms(partials, r)
        R.hold(f"stl_reduce_slabs nsplit {nsplit} entry {i}", a[sl].view(terms.shape[1:]), terms.double().sum(0), terms.sum(0))
    assert same_bits(a, exp)   # the gaps between the gradients hold the sentinel

    # the rows 1..2 alone: blk_base > 0, tab at the range's first entry
    rng = capi.ReduceRange()
    first, last = 1, 2
    rng.n, rng.blk_base, rng.nblocks = last - first + 1, rows[first]["blk0"], rows[last + 1]["blk0"] - rows[first]["blk0"]
    assert rng.blk_base > 0

    def part():
        grads = torch.full((ngrad,), R.SLAB_SENTINEL, device="cuda")
        rng.partials, rng.grads, rng.tab = pd.data_ptr(), grads.data_ptr(), tab.data_ptr() + first * C.sizeof(capi.Slab)
        capi.call("stl_reduce_slabs_range", C.byref(rng), stream())
        torch.cuda.synchronize()
        return grads
    c, d = part(), part()
    assert same_bits(c, d) and same_bits(c.cpu(), R.slab_ref(partials, rows, ngrad, F32, only=(first, last)))


# ------------------------------------------------------------------------------------------------ stl_head_forward / stl_head_backward
HEAD_FWD_DT = {"fp32": (capi.F32, F32), "bf16": (capi.BF16, BF16), "f16": (capi.F16, F16)}
HEAD_BWD_DT = {"fp32": (capi.F32, F32, F32), "bf16": (capi.BF16, BF16, BF16), "mixed": (capi.dt2(capi.BF16, capi.F16), BF16, F16)}   # code, dx, x


def nhwc(x, td):
    return x.permute(0, 2, 3, 1).contiguous().to(td).cuda()


@pytest.mark.parametrize("dt", list(HEAD_FWD_DT))
@pytest.mark.parametrize("pixels", list(R.HEAD_PIXELS))
@pytest.mark.parametrize("Ci", R.HEAD_CI + (24, 80))   # the forward kernel takes any multiple of 8
@pytest.mark.parametrize("J", R.HEAD_J)
def test_head_forward_is_conv2d(J, Ci, pixels, dt):
    code, td = HEAD_FWD_DT[dt]
    B, H, W = R.HEAD_PIXELS[pixels]
    x, w, bias, dout = R.head_data(J, Ci, pixels, td)
    xd, wd, bd = nhwc(x, td), w.cuda(), bias.cuda()

    def run(b):
        out = torch.full((B, J, H, W), NAN, device="cuda")
        capi.call("stl_head_forward", code, xd.data_ptr(), wd.data_ptr(), ptr(b), out.data_ptr(), B, H, W, Ci, J, stream())
        torch.cuda.synchronize()
        return out
    for b, zero in ((bd, 1.0), (None, 0.0)):
        got, again = run(b), run(b)
        assert same_bits(got, again) and not torch.isnan(got).any()
        y64, y32 = R.head_ref(x, w, bias * zero, dout, F64)[0], R.head_ref(x, w, bias * zero, dout, F32)[0]
        R.hold(f"stl_head_forward {dt} J {J} Ci {Ci} px {pixels} bias {b is not None}", got.cpu(), y64, y32)


@pytest.mark.parametrize("dt", list(HEAD_BWD_DT))
@pytest.mark.parametrize("pixels", list(R.HEAD_PIXELS))
@pytest.mark.parametrize("Ci", R.HEAD_CI)
@pytest.mark.parametrize("J", R.HEAD_J)
def test_head_backward_is_conv2d_autograd(J, Ci, pixels, dt):
    code, td, tx = HEAD_BWD_DT[dt]
    B, H, W = R.HEAD_PIXELS[pixels]
    P, nel = B * H * W, J * Ci + J
    x, w, bias, dout = R.head_data(J, Ci, pixels, tx)
    xd, wd, dd = nhwc(x, tx), w.cuda(), dout.cuda()
    (_, dx64, dw64, db64), (_, dx32, dw32, db32) = R.head_ref(x, w, bias, dout, F64), R.head_ref(x, w, bias, dout, F32)
    for nblk in R.HEAD_NBLK:
        def run():
            dx = torch.full((B, H, W, Ci), NAN, dtype=td, device="cuda")
            part = torch.full((nblk, nel), NAN, device="cuda")
            capi.call("stl_head_backward", code, xd.data_ptr(), wd.data_ptr(), dd.data_ptr(), dx.data_ptr(), part.data_ptr(), nblk,
                      B, H, W, Ci, J, stream())
            torch.cuda.synchronize()
            return dx, part
        (dx, part), (dx2, part2) = run(), run()
        assert same_bits(dx, dx2) and same_bits(part, part2)
        assert not torch.isnan(dx.float()).any() and not torch.isnan(part).any()
        nchunk = -(-P // 256)
        assert (part[nchunk:] == 0).all()   # blocks without a chunk write zeros
        tag = f"stl_head_backward {dt} J {J} Ci {Ci} px {pixels} nblk {nblk}"
        got = dx.cpu().permute(0, 3, 1, 2)
        if td == F32:
            R.hold(f"{tag} dx", got, dx64, dx32)
        else:
            R.hold16(f"{tag} dx", got, dx64, dx32, R.ROUND[td])
        s = part.cpu().double().sum(0)
        R.hold(f"{tag} dw", s[:J * Ci].view(J, Ci), dw64, dw32)
        R.hold(f"{tag} db", s[J * Ci:], db64, db32)


@pytest.mark.parametrize("J,Ci", [(15, 32), (17, 24), (17, 80)])
def test_head_refuses_what_it_cannot_run(J, Ci):
    B, H, W = 1, 4, 4
    x = torch.ones(B, H, W, Ci, device="cuda")
    w, bias = torch.ones(max(J, 17), Ci, device="cuda"), torch.ones(17, device="cuda")
    dout = torch.ones(B, max(J, 17), H, W, device="cuda")
    dx = torch.full((B, H, W, Ci), NAN, device="cuda")
    part = torch.full((2, 18 * Ci + 18), NAN, device="cuda")
    with pytest.raises(RuntimeError, match="head_bwd"):
        capi.call("stl_head_backward", capi.F32, x.data_ptr(), w.data_ptr(), dout.data_ptr(), dx.data_ptr(), part.data_ptr(), 2,
                  B, H, W, Ci, J, stream())
    torch.cuda.synchronize()
    assert torch.isnan(dx).all() and torch.isnan(part).all()   # refused, not run
    if J == 15:   # the forward kernel is built for 16 and 17 joints; it takes every Ci % 8 == 0 (test_head_forward_is_conv2d)
        out = torch.full((B, 17, H, W), NAN, device="cuda")
        with pytest.raises(RuntimeError, match="head: J=15"):
            capi.call("stl_head_forward", capi.F32, x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, Ci, J, stream())
        torch.cuda.synchronize()
        assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ stl_mse_loss / stl_sum_partials
LOSS_SENT = -3.5


@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("B,J,HW,nblk", [(3, 17, 35, 2),      # 1785 elements: no multiple of 256 * nblk
                                         (3, 17, 35, 16),     # 7 chunks of 256, 16 blocks
                                         (2, 16, 64, 3),
                                         (1, 17, 7, 1)])
def test_mse_loss_is_person_mse_loss(B, J, HW, nblk, gscale):
    o, t, tw = R.mse_data(B, J, HW)
    n = B * J * HW
    od, td_, wd = o.cuda(), t.cuda(), tw.cuda()
    (l64, d64), (l32, d32) = R.mse_ref(o, t, tw, gscale, F64), R.mse_ref(o, t, tw, gscale, F32)

    def run(with_loss=True, with_dout=True):
        def once():
            dout = torch.full((B, J, HW), NAN, device="cuda")
            partial = torch.full((nblk,), NAN, dtype=F64, device="cuda")
            loss = torch.full((1,), LOSS_SENT, device="cuda")
            capi.call("stl_mse_loss", od.data_ptr(), td_.data_ptr(), wd.data_ptr(), dout.data_ptr() if with_dout else None,
                      partial.data_ptr(), nblk, loss.data_ptr() if with_loss else None, B, J, HW, gscale, stream())
            torch.cuda.synchronize()
            return dout, partial, loss
        a, b = once(), once()
        for x, y in zip(a, b):
            assert same_bits(x, y)
        return a
    tag = f"stl_mse_loss B {B} J {J} HW {HW} nblk {nblk} gscale {gscale}"
    dout, partial, loss = run()
    assert not torch.isnan(partial).any() and (partial[-(-n // 256):] == 0).all()   # blocks without elements write 0
    R.hold(f"{tag} loss", loss[0].cpu(), l64, l32)
    R.hold(f"{tag} partials", partial.sum().cpu() * 0.5 / n, l64, l32)
    R.hold(f"{tag} dout", dout.cpu(), d64, d32)
    assert (dout[0, 1] == 0).all() and tw[0, 1] == 0                                 # a joint of weight 0: exactly 0
    # loss = NULL: the word is untouched, and the partials summed later give the same scalar
    dout2, partial2, loss2 = run(with_loss=False)
    assert loss2.item() == LOSS_SENT and same_bits(partial2, partial) and same_bits(dout2, dout)
    later = torch.full((1,), NAN, device="cuda")
    capi.call("stl_sum_partials", partial2.data_ptr(), nblk, 0.5 / n, later.data_ptr(), 0, stream())
    acc = torch.full((1,), 1.5, device="cuda")
    capi.call("stl_sum_partials", partial2.data_ptr(), nblk, 0.5 / n, acc.data_ptr(), 1, stream())
    torch.cuda.synchronize()
    assert same_bits(later, loss)
    R.hold(f"{tag} accumulated", acc[0].cpu(), l64 + 1.5, l32 + 1.5)
    # dout = NULL: the same sums, nothing written to the gradient
    dout3, partial3, loss3 = run(with_dout=False)
    assert torch.isnan(dout3).all() and same_bits(partial3, partial) and same_bits(loss3, loss)
