"""GPU: training the whole backbone with the BiFPN and the heads (``set_train_trunk(k)``; csrc/detector_trunk.hip,
stlpose_amd/detector_train.py) against the fp64 yardstick tests/detector_trunk_ref.py, in four groups: the three new entry points alone
(the two depthwise ones exactly on integers at every (k, s), with z and the stem's by the rule below); the gradients of single blocks of
D0 / D3 -- no expand layer, 3 x 3 / 2, 5 x 5 / 2, the skip -- and of the stem against the vector-Jacobian product fed the device's own
stored block input and ``tr.block_dy``; the chain of D0's last six blocks through a 5 x 5 / 2 block and the P4 join against
``method_yardstick``; and the whole model: "all", two runs, linearity, the optimiser step's refold, DetectorTrainer.

Bounds: the rule of tests/test_detector_train_gpu.py, nothing new.  Each figure is e = max|device - Y| / max|Y| of one tensor against
the fp64 yardstick Y and is held to max(MARGIN * e32, FLOOR), e32 being the same figure of the fp32 torch evaluation of the same
yardstick, MARGIN = 8, FLOOR = 1e-6.

A missing P4 join is seen: the yardstick is evaluated a second time with P4 detached where the first cell reads it, and the device's
gradients of block 10 must differ from that variant by more than the bound they are held to."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, detector_train as T, efficientdet as E
from tests import detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR, detector_trunk_ref as UR
from tests.test_detector_bifpn_first_gpu import LEVEL_NODES, _nchw
from tests.test_detector_train_gpu import MARGIN, TARGETS, _model

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATIOS = {}   # tensor class -> the largest e / e32 among its figures above the floor, printed by the tests that fill it
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bound(y32, y64):
    return max(MARGIN * TR.rel_err(y32, y64), TR.FLOOR)


def _hold(name, got, y64, y32, cls=None):
    """Print the figures, then hold e to max(MARGIN * e32, FLOOR)."""
    e, e32 = TR.rel_err(got, y64), TR.rel_err(y32, y64)
    ratio = e / e32 if e32 else float("inf") if e else 0.0
    print(f"{name}: e {e:.3e} e32 {e32:.3e} ratio {ratio:.2f}")
    if cls is not None and e > TR.FLOOR:
        RATIOS[cls] = max(RATIOS.get(cls, 0.0), ratio)
    assert e <= max(MARGIN * e32, TR.FLOOR), (name, e, e32)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


# ------------------------------------------------------------------------------------------------ the two depthwise entry points alone
def _dw_data(dy, w, z, dx, B, H, W, C, k, s):
    capi.call("stl_det_dwconv_bwd_data_ks", _ptr(dy), _ptr(w), _ptr(z), _ptr(dx), B, H, W, C, k, s, _st())
    torch.cuda.synchronize()


def _dw_weight(x, dy, part, dw, B, H, W, C, k, s):
    capi.call("stl_det_dwconv_bwd_weight_ks", _ptr(x), _ptr(dy), _ptr(part), _ptr(dw), B, H, W, C, k, s, _st())
    torch.cuda.synchronize()


def _dw_case(B, H, W, C, k, s, integers, seed):
    """x, w [C, k, k], dy, z in NCHW on the host; integers: every value an integer with |v| <= 4."""
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = -(-H // s), -(-W // s)
    if integers:
        mk = lambda *shape: torch.randint(-4, 5, shape, generator=gen).double()  # noqa: E731
    else:
        mk = lambda *shape: torch.randn(*shape, generator=gen).float().double()  # noqa: E731
    return mk(B, C, H, W), mk(C, k, k), mk(B, C, Ho, Wo), mk(B, C, H, W)


def _dw_device(x, w, dy, z, k, s):
    """dx and dw of the two entry points, twice -> [(dx NCHW, dw [C, k, k]), ...] on the host; the outputs start as NaN."""
    B, C, H, W = x.shape
    xd, dyd, wd = _nhwc(x), _nhwc(dy), w.permute(1, 2, 0).contiguous().float().to(DEV)
    zd = None if z is None else _nhwc(z)
    parts = capi.lib().stl_det_dwconv_bwd_ks_parts(B * dy.shape[2] * dy.shape[3])
    outs = []
    for _ in range(2):
        dx, dw, part = _nan(B, H, W, C), _nan(k, k, C), _nan(parts * k * k * C)
        _dw_data(dyd, wd, zd, dx, B, H, W, C, k, s)
        _dw_weight(xd, dyd, part, dw, B, H, W, C, k, s)
        outs.append((dx.permute(0, 3, 1, 2).cpu(), dw.permute(2, 0, 1).cpu()))
    return outs


SMALL = [(2, 7, 6), (2, 6, 7), (3, 1, 1), (2, 2, 3)]   # both parities in both axes; a single pixel; a map smaller than the kernel


@pytest.mark.parametrize("k,s", KS)
@pytest.mark.parametrize("C", [8, 72])
def test_depthwise_backward_is_exact_on_integers(k, s, C):
    """|values| <= 4 and at most 1275 pixels: every product and sum is an integer below 2^24, exact in fp32 in any order.  same_pad_before
    at s = 2 is 0 / 1 / 1 / 2 for k3-even / k3-odd / k5-even / k5-odd, and (7, 6) / (6, 7) have both in both axes."""
    if s == 2:
        assert [UR.same_pad_before(n, k, 2) for n in (6, 7)] == ({3: [0, 1], 5: [1, 2]}[k])
    big = (5, 17, 15) if s == 1 else (5, 16, 15)   # more than one pixel range, the last one ragged
    npix = big[0] * -(-big[1] // s) * -(-big[2] // s)
    parts = capi.lib().stl_det_dwconv_bwd_ks_parts(npix)
    assert parts > 1 and npix % -(-npix // parts), (npix, parts)
    for B, H, W in SMALL + ([big] if C == 8 else []):
        x, w, dy, _ = _dw_case(B, H, W, C, k, s, True, 100 * k + 10 * s + H + C)
        dx64, dw64 = UR.dw_autograd(x, w, dy, k, s)
        outs = _dw_device(x, w, dy, None, k, s)
        assert torch.equal(outs[0][0].double(), dx64), ("dx", B, H, W)
        assert torch.equal(outs[0][1].double(), dw64), ("dw", B, H, W)
        assert all(torch.equal(a, b) for a, b in zip(*outs)), "two runs differ"


@pytest.mark.parametrize("k,s", KS)
def test_depthwise_data_backward_with_z(k, s):
    for (B, H, W), C in zip(SMALL + [(5, 16, 15)], (8, 72, 8, 72, 8)):
        x, w, dy, z = _dw_case(B, H, W, C, k, s, False, 7 * k + s + W)
        z = z * 2
        dx64, _ = UR.dw_autograd(x, w, dy, k, s, z)
        dx32, _ = UR.dw_autograd(x.float(), w.float(), dy.float(), k, s, z.float())
        outs = _dw_device(x, w, dy, z, k, s)
        _hold(f"dwconv_bwd_data_ks k{k} s{s} {B}x{H}x{W}x{C} dx", outs[0][0], dx64, dx32)
        assert torch.equal(outs[0][0], outs[1][0]), "two runs differ"


def test_depthwise_backward_checks_its_arguments():
    B, H, W, C, k, s = 2, 6, 7, 8, 5, 2
    Ho, Wo = 3, 4
    dy, z = torch.zeros(B, Ho, Wo, C, device=DEV), torch.zeros(B, H, W, C, device=DEV)
    w, x = torch.zeros(k, k, C, device=DEV), torch.zeros(B, H, W, C, device=DEV)
    dx, dw = torch.full((B, H, W, C), 7.0, device=DEV), torch.full((k, k, C), 7.0, device=DEV)
    part = torch.full((capi.lib().stl_det_dwconv_bwd_ks_parts(B * Ho * Wo) * k * k * C,), 7.0, device=DEV)
    for bad in (0, 1, 3):   # z may be null
        args = [dy, w, z, dx]
        args[bad] = None
        with pytest.raises(RuntimeError, match="det_dwconv_bwd_data_ks: null pointer"):
            _dw_data(*args, B, H, W, C, k, s)
    for bad in range(4):
        args = [x, dy, part, dw]
        args[bad] = None
        with pytest.raises(RuntimeError, match="det_dwconv_bwd_weight_ks: null pointer"):
            _dw_weight(*args, B, H, W, C, k, s)
    for name, run in (("data", lambda *d: _dw_data(dy, w, z, dx, *d)), ("weight", lambda *d: _dw_weight(x, dy, part, dw, *d))):
        for dims in ((0, H, W, C, k, s), (B, 0, W, C, k, s), (B, H, -1, C, k, s), (B, H, W, 0, k, s)):
            with pytest.raises(RuntimeError, match=f"det_dwconv_bwd_{name}_ks: B"):
                run(*dims)
        for kk, ss in ((4, 1), (7, 1), (1, 1), (3, 3), (5, 0)):
            with pytest.raises(RuntimeError, match=f"det_dwconv_bwd_{name}_ks: k {kk} s {ss}"):
                run(B, H, W, C, kk, ss)
        for cc in (6, 9, 2):
            with pytest.raises(RuntimeError, match=f"det_dwconv_bwd_{name}_ks: C {cc}"):
                run(B, H, W, cc, k, s)
    with pytest.raises(RuntimeError, match="det_dwconv_bwd_data_ks: a pointer is not 16-byte aligned"):
        _dw_data(dy.view(-1)[1:], w, z, dx, 1, H, W, C, k, s)
    both = torch.full((2 * B * H * W * C,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="det_dwconv_bwd_data_ks: dx overlaps"):
        _dw_data(both[8:], w, z, both, B, H, W, C, k, s)
    with pytest.raises(RuntimeError, match="det_dwconv_bwd_weight_ks: partial or dw overlaps"):
        _dw_weight(x, dy, part, part[16:], B, H, W, C, k, s)
    with pytest.raises(RuntimeError, match="det_dwconv_bwd_weight_ks: partial or dw overlaps"):
        _dw_weight(both, dy, both[16:], dw, B, H, W, C, k, s)
    assert all(bool((t == 7.0).all()) for t in (dx, dw, part, both)), "a refused call wrote something"
    assert capi.lib().stl_det_dwconv_bwd_ks_parts(0) == 0 and capi.lib().stl_det_stem_bwd_parts(-3) == 0


# ------------------------------------------------------------------------------------------------ stl_det_stem_bwd alone
def _stem_ref(x, w, b, dy, dtype):
    """x NCHW, w [Co, 3, 3, 3], b [Co]: swish(conv / 2 under TF-same padding + b).backward(dy) -> (dw [3][3][3][Co], db)."""
    x, dy = x.to(dtype), dy.to(dtype)
    w, b = w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
    F.silu(F.conv2d(R._same(x, 3, 2), w, b, 2)).backward(dy)
    return w.grad.permute(2, 3, 1, 0).contiguous(), b.grad


def _stem(x, w, b, dy, part, dw, db, B, H, W, Co):
    capi.call("stl_det_stem_bwd", _ptr(x), _ptr(w), _ptr(b), _ptr(dy), _ptr(part), _ptr(dw), _ptr(db), B, H, W, Co, _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H,W,Co", [(2, 9, 8, 40), (3, 33, 30, 32)])   # one pixel range; six, the last one ragged
def test_stem_backward(B, H, W, Co):
    gen = torch.Generator().manual_seed(H + Co)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x, dy = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, Co, Ho, Wo, generator=gen)
    w, b = torch.randn(Co, 3, 3, 3, generator=gen) / 27 ** 0.5, torch.randn(Co, generator=gen) * 0.3
    (dw64, db64), (dw32, db32) = _stem_ref(x, w, b, dy, torch.float64), _stem_ref(x, w, b, dy, torch.float32)
    parts = capi.lib().stl_det_stem_bwd_parts(B * Ho * Wo)
    assert (parts > 1) == (B == 3) and (B != 3 or (B * Ho * Wo) % -(-(B * Ho * Wo) // parts))
    xd, dyd, wd, bd = _nhwc(x), _nhwc(dy), w.permute(2, 3, 1, 0).contiguous().to(DEV), b.to(DEV)
    outs = []
    for _ in range(2):
        part, dw, db = _nan(parts * 28 * Co), _nan(3, 3, 3, Co), _nan(Co)
        _stem(xd, wd, bd, dyd, part, dw, db, B, H, W, Co)
        outs.append((dw.cpu(), db.cpu()))
    _hold(f"stem_bwd {B} {H}x{W} {Co} dw", outs[0][0], dw64, dw32)
    _hold(f"stem_bwd {B} {H}x{W} {Co} db", outs[0][1], db64, db32)
    assert all(torch.equal(a, c) for a, c in zip(*outs)), "two runs differ"


def test_stem_backward_checks_its_arguments():
    B, H, W, Co = 2, 9, 8, 8
    x, dy = torch.zeros(B, H, W, 3, device=DEV), torch.zeros(B, 5, 4, Co, device=DEV)
    w, b = torch.zeros(27 * Co, device=DEV), torch.zeros(Co, device=DEV)
    part = torch.full((capi.lib().stl_det_stem_bwd_parts(B * 20) * 28 * Co,), 7.0, device=DEV)
    dw, db = torch.full((27 * Co,), 7.0, device=DEV), torch.full((Co,), 7.0, device=DEV)
    for bad in range(7):
        args = [x, w, b, dy, part, dw, db]
        args[bad] = None
        with pytest.raises(RuntimeError, match="det_stem_bwd: null pointer"):
            _stem(*args, B, H, W, Co)
    for dims in ((0, H, W, Co), (B, 0, W, Co), (B, H, 0, Co), (B, H, W, 0)):
        with pytest.raises(RuntimeError, match="det_stem_bwd: B"):
            _stem(x, w, b, dy, part, dw, db, *dims)
    with pytest.raises(RuntimeError, match="det_stem_bwd: partial, dw or db overlaps"):
        _stem(x, w, b, dy, part, part[16:], db, B, H, W, Co)
    with pytest.raises(RuntimeError, match="det_stem_bwd: partial, dw or db overlaps"):
        _stem(x, w, b, dy, part, w, db, B, H, W, Co)
    assert all(bool((t == 7.0).all()) for t in (part, dw, db)), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ the model
def _chw(n):
    return [torch.from_numpy(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255)) for im in R.images()[:n]]


def _step(m, chw, targets):
    """One detection_loss + backward -> (losses, {parameter: grad})."""
    for q in m.parameters():
        q.grad = None
    loss = m.detection_loss(chw, targets)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    return ({n: v.detach().clone() for n, v in loss.items()},
            {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None})


def _check_block(o, i, tag):
    """Every parameter gradient of block i against the vector-Jacobian product of the yardstick's block, fed the device's own stored
    block input and the gradient of the block's output the device formed (after its joins)."""
    spec, plan, tr = E.block_specs(o["cc"])[i], o["plan"], o["plan"].train
    x, dy = _nchw(plan.blocks[i][0]), _nchw(tr.block_dy[i])
    assert dy.shape == _nchw(plan.blocks[i][4]).shape and bool(dy.abs().max() > 0)
    g64, _ = UR.block_vjp(o["sd"], i, spec, x, dy, torch.float64)
    g32, _ = UR.block_vjp(o["sd"], i, spec, x, dy, torch.float32)
    assert len(g64) == (10 if spec["e"] == 1 else 13)
    for name in g64:
        got = o["grads"][name]
        assert got.shape == g64[name].shape and bool(got.abs().max() > 0), name
        _hold(f"{tag} {name}", got, g64[name], g32[name], UR.tensor_class(name))


@pytest.fixture(scope="module")
def d0_all():
    """D0 at batch 1, everything trains.  The targets are D3's five boxes on the first image: 31 to 400 pixels, so every pyramid level
    has positive anchors and every BN of the regressor a gradient."""
    m, sd = _model(0)
    chw, targets = _chw(1), TARGETS[3]
    m.set_train_bifpn("all").set_train_trunk("all")
    plan = m.plan(1, DEV)
    loss, grads = _step(m, chw, targets)
    assert m.plan(1, DEV) is plan and plan.train is not None
    return dict(m=m, sd=sd, cc=0, chw=chw, targets=targets, plan=plan, loss=loss, grads=grads)


@pytest.mark.parametrize("i", [0, 1, 3, 11])
def test_d0_single_block_gradients(d0_all, i):
    """Block 0 has no expand layer, block 1 is 3 x 3 / 2 on 256 x 256, block 3 is 5 x 5 / 2 on 128 x 128, block 11 is 5 x 5 / 2 and
    reads P4."""
    specs = E.block_specs(0)
    assert [(specs[j]["e"], specs[j]["k"], specs[j]["s"]) for j in (0, 1, 3, 11)] == [(1, 3, 1), (6, 3, 2), (6, 5, 2), (6, 5, 2)]
    assert d0_all["plan"].blocks[3][0].shape[1] == 128 and d0_all["plan"].blocks[11][0] is d0_all["plan"].backbone[1]
    _check_block(d0_all, i, f"d0 block {i}")
    print("ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


def test_d0_stem_gradients(d0_all):
    plan, tr = d0_all["plan"], d0_all["plan"].train
    assert tr.stem_dy.shape == plan.blocks[0][0].shape
    x, dy = _nchw(plan.canvas), _nchw(tr.stem_dy)
    g64, g32 = UR.stem_vjp(d0_all["sd"], x, dy, torch.float64), UR.stem_vjp(d0_all["sd"], x, dy, torch.float32)
    assert len(g64) == 3
    for name in g64:
        got = d0_all["grads"][name]
        assert got.shape == g64[name].shape and bool(got.abs().max() > 0), name
        _hold(f"d0 stem {name}", got, g64[name], g32[name], UR.tensor_class(name))
    print("ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


def test_stem_gradients_read_the_canvas_of_a_det_batch():
    """A DetBatch brings a canvas of its own, which the forward's stem reads where it lies; the stem's backward must read the same one,
    and the plan's own again for the next host-fed call.  The plan's own canvas holds other pixels (the first image twice), so the
    vector-Jacobian product on the wrong canvas lies outside the bound, which the test asserts too."""
    from tests import test_det_batch_gpu as DB
    m = DB._model(train_header=True).set_train_bifpn("all").set_train_trunk("all")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    batch, _, _ = DB._model_batch(512)
    host = [_chw(1)[0]] * 2
    targets = [TARGETS[3][0]] * 2
    _step(m, host, targets)
    plan = m.plan(2, DEV)
    own, other = plan.canvas, batch.canvas
    assert other.data_ptr() != own.data_ptr() and other.shape == own.shape and not torch.equal(other, own)
    names = ("backbone_net.model._conv_stem.conv.weight", "backbone_net.model._bn0.weight", "backbone_net.model._bn0.bias")
    for tag, args, canvas, wrong in (("batch", (batch, None), other, own), ("host again", (host, targets), own, other)):
        for q in m.parameters():
            q.grad = None
        sum(m.detection_loss(*args).values()).backward()
        torch.cuda.synchronize()
        assert m.plan(2, DEV) is plan
        dy = _nchw(plan.train.stem_dy)
        g64, g32 = UR.stem_vjp(sd, _nchw(canvas), dy, torch.float64), UR.stem_vjp(sd, _nchw(canvas), dy, torch.float32)
        gbad = UR.stem_vjp(sd, _nchw(wrong), dy, torch.float64)
        for name in names:
            got = dict(m.named_parameters())[name].grad
            _hold(f"stem, {tag} {name}", got, g64[name], g32[name], UR.tensor_class(name))
            gap = (got.cpu().double() - gbad[name]).abs().max().item() / g64[name].abs().max().item()
            print(f"stem, {tag} {name}: against the other canvas {gap:.3e}")
            assert gap > _bound(g32[name], g64[name]), (name, gap)


def test_d0_all_reaches_every_parameter_and_two_runs_are_bitwise_equal(d0_all):
    m = d0_all["m"]
    assert m.train_stem and m.train_backbone == 16
    names = {n for n, _ in m.named_parameters()}
    assert set(d0_all["grads"]) == names == {n for n, _ in T.trainable_parameters(m)}
    for n, g in d0_all["grads"].items():
        assert bool(torch.isfinite(g).all()) and bool(g.abs().max() > 0), n
    loss, grads = _step(m, d0_all["chw"], d0_all["targets"])
    assert all(torch.equal(loss[n], d0_all["loss"][n]) for n in loss) and set(grads) == names
    for n, g in d0_all["grads"].items():
        assert torch.equal(grads[n], g), n


def test_d3_block_without_an_expand_layer_with_the_skip():
    """D3's block 1: e = 1 and the identity skip, so block 0 trains through the depthwise data gradient plus dy itself."""
    m, sd = _model(3)
    specs = E.block_specs(3)
    assert specs[1]["e"] == 1 and specs[1]["skip"] and specs[0]["e"] == 1 and not specs[0]["skip"]
    chw, targets = _chw(1), TARGETS[3]
    m.set_train_bifpn("all").set_train_trunk(26)
    plan = m.plan(1, DEV)
    loss, grads = _step(m, chw, targets)
    assert not any(n.startswith("backbone_net.model._conv_stem") for n in grads) and plan.train.stem_dy is None
    o = dict(m=m, sd=sd, cc=3, plan=plan, grads=grads)
    _check_block(o, 1, "d3 block 1")
    _check_block(o, 0, "d3 block 0")
    print("ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


# ------------------------------------------------------------------------------------------------ the chain
# the parent's backward launches of one final-stage block behind the P5 join, in order
PARENT_BLOCK = ["stl_det_pointwise_bwd_data", "stl_det_mbconv_gate_bwd", "stl_det_pointwise_bwd_weight", "stl_det_se_bwd", "stl_det_dwconv",
                "stl_det_mbconv_act_bwd", "stl_det_dwconv_bwd_weight", "stl_det_pointwise", "stl_det_dwconv_bwd_data",
                "stl_det_pointwise_bwd_weight"]
PARENT_P5 = ["stl_det_pointwise_bwd_data"] * 3 + ["stl_det_grad_add"] * 2


@pytest.fixture(scope="module")
def d0_chain():
    """D0 on the two test images; one run per k: none, the final stage through either setter, the last six blocks, the last seven."""
    m, sd = _model(0)
    targets = TARGETS[0]
    chw = _chw(len(targets))
    o = dict(m=m, sd=sd, cc=0, chw=chw, targets=targets, runs={})
    o["plan"] = plan = m.plan(len(chw), DEV)
    m.set_train_bifpn("all")
    for tag, setter, k in (("0", m.set_train_trunk, 0), ("bb1", m.set_train_backbone, 1), ("1", m.set_train_trunk, 1), ("6", m.set_train_trunk, 6),
                           ("7", m.set_train_trunk, 7)):
        setter(k)
        loss, grads = _step(m, chw, targets)
        assert m.plan(len(chw), DEV) is plan
        tr = plan.train
        o["runs"][tag] = dict(loss=loss, grads=grads, reg=tr.reg.clone(), cls=tr.cls.clone(), want=[n for n, _ in T.trainable_parameters(m)],
                              names=tr.bwd.names(), start=getattr(tr, "blocks_start", len(tr.bwd)),
                              block_dy={i: t.clone() for i, t in getattr(tr, "block_dy", {}).items()})
    o["levels"] = [[_nchw(kept[n][2]) for n in LEVEL_NODES] for kept in plan.cells]
    o["p34"] = [_nchw(f) for f in plan.backbone[:2]]
    o["t"], o["p6"] = _nchw(plan.first_pools[0][1]), _nchw(plan.first_pools[0][2])
    o["inputs"] = [_nchw(rec[0]) for rec in plan.blocks]
    gt, offsets = T.pack_targets(targets, [tuple(c.shape[1:]) for c in chw], 1)
    o["loss_args"] = (torch.from_numpy(m.anchors_np), torch.from_numpy(gt), offsets.tolist())
    return o


def test_d0_last_six_blocks_match_the_yardstick_through_the_p4_join(d0_chain):
    o = d0_chain
    specs = E.block_specs(0)
    blocks = list(range(10, 16))
    assert (specs[11]["k"], specs[11]["s"]) == (5, 2) and all(specs[i]["k"] == 5 and specs[i]["skip"] for i in (12, 13, 14))
    assert o["plan"].blocks[11][0] is o["plan"].backbone[1] and o["inputs"][10].shape[2] == 32 and o["inputs"][15].shape[2] == 16
    n = len(o["levels"])
    routes = {j: dict(zip(BR.POOLED, o["levels"][j][:4])) for j in range(n)}
    routes[0].update(t=o["t"], p6=o["p6"])
    args = (o["sd"], 0, 1, n, blocks, o["inputs"][10], o["p34"], routes, *o["loss_args"])
    c64, r64, g64 = UR.method_yardstick(*args, torch.float64)
    c32, r32, g32 = UR.method_yardstick(*args, torch.float32)
    _, _, gcut = UR.method_yardstick(*args, torch.float64, cut_p4=True)
    run = o["runs"]["6"]
    _hold("d0 k6 classification", run["loss"]["classification"], c64, c32)
    _hold("d0 k6 regression", run["loss"]["regression"], r64, r32)
    assert set(run["grads"]) == set(run["want"]) == set(g64), "a gradient outside trainable_parameters, or one missing"
    mine = [name for name in run["want"] if name.startswith("backbone_net.")]
    assert len(mine) == 13 * 6 and all(name.startswith(tuple(f"{UR.PRE}{i}." for i in blocks)) for name in mine)
    seen = 0
    for name in mine:
        got = run["grads"][name]
        assert got.shape == g64[name].shape and bool(got.abs().max() > 0), name
        _hold(f"d0 k6 {name}", got, g64[name], g32[name], UR.tensor_class(name))
        if name.startswith(f"{UR.PRE}10."):   # the test sees a missing P4 join
            gap = (got.cpu().double() - gcut[name]).abs().max().item() / g64[name].abs().max().item()
            print(f"d0 k6 {name}: against the variant without the P4 join {gap:.3e}")
            assert gap > _bound(g32[name], g64[name]), (name, gap)
            seen += 1
    assert seen == 13
    for name in mine:   # and the blocks behind P4 do not see the join at all
        if not name.startswith(f"{UR.PRE}10."):
            assert torch.equal(gcut[name], g64[name]), name
    print("d0 k6 ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


def test_d0_nothing_that_exists_moves(d0_chain):
    """Losses, reg, cls and every BiFPN / head gradient are those of k = 0 bit for bit at any k; a block's gradients do not depend on
    whether the blocks in front of it train; the gradient of a block's output neither."""
    runs = d0_chain["runs"]
    base = runs["0"]
    assert len(base["grads"]) > 100 and all(n.startswith(("bifpn.", "regressor.", "classifier.")) for n in base["grads"])
    for tag in ("bb1", "1", "6", "7"):
        run = runs[tag]
        assert all(torch.equal(run["loss"][n], base["loss"][n]) for n in ("classification", "regression"))
        assert torch.equal(run["reg"], base["reg"]) and torch.equal(run["cls"], base["cls"])
        assert set(base["grads"]) == {n for n in run["grads"] if not n.startswith("backbone_net.")}
        for n, g in base["grads"].items():
            assert torch.equal(run["grads"][n], g), (tag, n)
    for small, large in (("bb1", "1"), ("1", "6"), ("6", "7")):
        assert len(runs[small]["grads"]) <= len(runs[large]["grads"])
        for n, g in runs[small]["grads"].items():
            assert torch.equal(runs[large]["grads"][n], g), (small, large, n)
        for i, t in runs[small]["block_dy"].items():
            assert torch.equal(runs[large]["block_dy"][i], t), (small, large, i)
    assert sum(n.startswith(f"{UR.PRE}9.") for n in runs["7"]["grads"]) == 13 and not any(n.startswith(f"{UR.PRE}9.") for n in runs["6"]["grads"])


def test_d0_final_stage_backward_launches_are_the_parents(d0_chain):
    runs = d0_chain["runs"]
    for tag in ("bb1", "1"):
        names, start = runs[tag]["names"], runs[tag]["start"]
        assert names[:start] == runs["0"]["names"], "the heads' and the cells' launches changed"
        assert names[start:] == PARENT_P5 + PARENT_BLOCK, tag
    assert runs["bb1"]["names"] == runs["1"]["names"]
    # deeper blocks: the same sequence with the _ks entry points, the input's data gradient and its joins in front of the next block
    names, start = runs["6"]["names"], runs["6"]["start"]
    assert names[start:start + 15] == PARENT_P5 + PARENT_BLOCK
    ks = [n.replace("stl_det_dwconv_bwd_weight", "stl_det_dwconv_bwd_weight_ks").replace("stl_det_dwconv_bwd_data", "stl_det_dwconv_bwd_data_ks")
          for n in PARENT_BLOCK]
    rest = names[start + 15:]
    assert rest[0] == "stl_det_pointwise_bwd_data" and rest[1:11] == ks   # block 15's dx (it has no skip), then block 14
    assert rest[11:13] == ["stl_det_pointwise_bwd_data", "stl_det_grad_add"]   # block 14's dx and its skip
    assert names.count("stl_det_dwconv_bwd_weight_ks") == 5 and names.count("stl_det_dwconv_bwd_data_ks") == 5
    assert names.count("stl_det_grad_add") == runs["0"]["names"].count("stl_det_grad_add") + 2 + 3 + 2   # P5; the skips of 14, 13, 12; P4


# ------------------------------------------------------------------------------------------------ the whole model
def test_sgd_step_keeps_the_plan_and_refolds_everything_in_place_exactly(d0_all):
    m, plan = d0_all["m"], d0_all["plan"]
    m.set_train_bifpn("all").set_train_trunk("all")
    _step(m, d0_all["chw"], d0_all["targets"])
    wbuf, before = m._wbuf, m._wbuf.clone()
    params = [q for _, q in T.trainable_parameters(m)]
    assert len(params) == len(list(m.parameters())) and all(q.grad is not None for q in params)
    torch.optim.SGD(params, lr=1e-3).step()
    assert m.plan(1, DEV) is plan and m._wbuf is wbuf and plan.train is not None
    fresh = E.setup_detector("efficientdet", "d0")
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.to(DEV).ready(DEV)
    assert torch.equal(m._wbuf, fresh._wbuf)
    stem_w, stem_b = m._layout["stem"]
    assert stem_w == 0 and not torch.equal(m._wbuf[:stem_b], before[:stem_b]) and not torch.equal(m._wbuf[stem_b:m._block_off[0][0]],
                                                                                                   before[stem_b:m._block_off[0][0]])
    for i in range(16):   # every block moved
        lo, hi = m._block_off[i][0], m._block_off[i + 1][0] if i < 15 else m._tail_off[0][0]
        assert not torch.equal(m._wbuf[lo:hi], before[lo:hi]), i
    again, _ = _step(m, d0_all["chw"], d0_all["targets"])
    assert all(bool(torch.isfinite(v)) for v in again.values())
    assert not torch.equal(again["classification"], d0_all["loss"]["classification"])   # the step moved the network
    # a step with blocks but without the stem refolds from the first trainable block on
    m.set_train_trunk(9)
    _step(m, d0_all["chw"], d0_all["targets"])
    before = m._wbuf.clone()
    torch.optim.SGD([q for _, q in T.trainable_parameters(m)], lr=1e-3).step()
    assert m.plan(1, DEV) is plan and m._wbuf is wbuf
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.ready(DEV)
    first = m._block_off[7][0]
    assert torch.equal(m._wbuf, fresh._wbuf) and torch.equal(m._wbuf[:first], before[:first]) and not torch.equal(m._wbuf[first:], before[first:])


def test_loss_weights_reach_the_trunk():
    """Every trunk gradient is linear in the two losses' gradients: 2 * classification + 0.5 * regression."""
    m, _ = _model(0)
    m.set_train_bifpn("all").set_train_trunk("all")
    chw, targets = _chw(1), TARGETS[3]
    grads = {}
    for tag, (wc, wr) in (("c", (1.0, 0.0)), ("r", (0.0, 1.0)), ("mix", (2.0, 0.5))):
        for q in m.parameters():
            q.grad = None
        loss = m.detection_loss(chw, targets)
        (wc * loss["classification"] + wr * loss["regression"]).backward()
        grads[tag] = {n: q.grad.clone() for n, q in T.trainable_parameters(m) if n.startswith("backbone_net.")}
    assert len(grads["mix"]) == 3 + 10 + 13 * 15
    for n, g in grads["mix"].items():
        want = 2.0 * grads["c"][n].double() + 0.5 * grads["r"][n].double()
        assert bool(want.abs().max() > 0) and (g.double() - want).abs().max() <= 1e-4 * want.abs().max() + 1e-12, n


def test_detector_trainer_trains_the_whole_trunk_and_resumes(tmp_path):
    from stlpose_amd.det_data import DetBatchLoader
    from stlpose_amd.detector_trainer import DetectorTrainer
    from stlpose_amd.pose_data import ResidentImages
    from tests import test_det_batch_gpu as DB
    images, db = DB._images(DB.T_SIZES, 21), DB._db(DB.T_SIZES, DB.T_BOXES, DB.T_LABELS)
    store = ResidentImages.from_arrays(images, DEV)

    def trainer(exp_path, **kw):
        exp = DB._exp_data()
        exp["training"]["train_bifpn"] = "all"
        exp["training"]["train_trunk"] = "all"
        model = DB._model(train_header=True)
        train, valid = DetBatchLoader(db, store, exp, 2, True, seed=3), DetBatchLoader(db, store, exp, 2, False)
        return DetectorTrainer(str(exp_path), exp, model, train, valid, db.coco_gt(256), valid_fraction=1.0, **kw)
    t = trainer(tmp_path / "full")
    nblocks = len(t.model.backbone_net.model._blocks)
    assert t.model.train_bifpn == 3 and t.model.train_backbone == nblocks and t.model.train_stem
    optimised = {id(q) for group in t.optimizer.param_groups for q in group["params"]}
    assert optimised == {id(q) for _, q in T.trainable_parameters(t.model)} == {id(q) for q in t.model.parameters()}
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    t.training_loop()
    logs = json.loads((tmp_path / "full" / "detector_logs.json").read_text())
    assert len(logs["train_loss"]) == 2 and t.skipped == 0 and all(np.isfinite(logs["train_loss"]))
    after = t.model.state_dict()
    params = {n for n, _ in t.model.named_parameters()}
    for k, v in after.items():
        if k.startswith("backbone_net.") and k in params:
            assert not torch.equal(v, before[k]), k          # the stem and every block move, every parameter of them
        elif k not in params:
            assert torch.equal(v, before[k]), k              # every buffer stays
    saved = tmp_path / "full" / "models" / "detector"
    os.makedirs(tmp_path / "resumed")
    shutil.copy(tmp_path / "full" / "detector_logs.json", tmp_path / "resumed" / "detector_logs.json")
    r = trainer(tmp_path / "resumed", checkpoint=str(saved / "checkpoint_epoch_0.pth"), resume_training=True)
    assert r.cur_epoch == 1 and r.model.train_stem and r.model.train_backbone == nblocks
    r.training_loop()
    for k, v in after.items():
        assert torch.equal(v, r.model.state_dict()[k]), k
