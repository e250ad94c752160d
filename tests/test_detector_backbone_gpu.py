"""GPU: training the backbone's last stage with the BiFPN and the heads (``set_train_backbone(k)``; csrc/detector_mbconv.hip,
stlpose_amd/detector_train.py) against the fp64 yardstick tests/detector_backbone_ref.py: the three new entry points alone
(stl_det_mbconv_gate_bwd exactly, stl_det_se_bwd and stl_det_mbconv_act_bwd by the rule below),
EfficientDetBackbone.detection_loss end to end (D0 on the two test images with k = 1, D3 on one with k = 2), the optimiser step's
refold from the first trainable block, linearity in the two losses and DetectorTrainer.

Bounds: the rule of tests/test_detector_train_gpu.py, nothing new.  Each figure is e = max|device - Y| / max|Y| of one tensor against
the fp64 yardstick Y and is held to max(MARGIN * e32, FLOOR), e32 being the same figure of the fp32 torch evaluation of the same
yardstick with the same pool routing (the device's own stored fp32 maps), MARGIN = 8, FLOOR = 1e-6.

A missing gate path is seen: the yardstick is evaluated a second time with the squeeze-excitation gate held constant, and the device's
expand, depthwise and SE gradients must differ from that variant by more than the bound they are held to.  With
``synth_state_dict``'s weights the gate's share of the expand and depthwise gradients is 2.5 - 5.3 % for D0 and 1.7 - 3.0 % for D3
(fp64 against fp64, measured on the CPU first) and all of the SE gradients, against bounds near 1e-5, so ``_se_expand`` is used as
it is, unscaled.  The measured ratios per tensor class are in DESIGN.md ("Training the backbone's last stage")."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, detector_train as T, efficientdet as E
from tests import detector_backbone_ref as KR, detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR
from tests.test_detector_bifpn_first_gpu import LEVEL_NODES, _nchw
from tests.test_detector_train_gpu import MARGIN, TARGETS, _model

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATIOS = {}   # tensor class -> the largest e / e32 among its figures above the floor, printed by the tests that fill it


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


# ------------------------------------------------------------------------------------------------ stl_det_mbconv_gate_bwd alone
GATE_SHAPES = [(2, 1, 6), (2, 9, 8), (1, 256, 1152), (2, 784, 1392)]   # the scalar path, one pixel range, D0, D3's width on 28 x 28


def _gate(a, D, g, xs, ws, asum, dgate, B, HW, C):
    capi.call("stl_det_mbconv_gate_bwd", _ptr(a), _ptr(D), _ptr(g), _ptr(xs), _ptr(ws), _ptr(asum), _ptr(dgate), B, HW, C, _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,HW,C", GATE_SHAPES)
def test_gate_backward_is_exact_on_integers(B, HW, C):
    """|values| <= 3 and HW <= 784: every product and sum is an integer below 2^24, exact in fp32 in any order."""
    gen = torch.Generator().manual_seed(HW * 7 + C)
    a, D = (torch.randint(-3, 4, (B, HW, C), generator=gen).float() for _ in range(2))
    g = torch.randint(-3, 4, (B, C), generator=gen).float()
    lib = capi.lib()
    assert (lib.stl_det_mbconv_parts(HW) > 1) == (HW > 16)
    if (B, HW, C) == GATE_SHAPES[-1]:
        assert C % 64 and lib.stl_det_mbconv_parts(HW) == 16, "more than one workgroup per (image, channel range)"
    ad, Dd, gd = a.to(DEV), D.to(DEV), g.to(DEV)
    outs = []
    for _ in range(2):
        xs, asum, dgate = _nan(B, HW, C), _nan(B, C), _nan(B, C)
        ws = _nan(lib.stl_det_mbconv_gate_bwd_workspace(B, HW, C))
        _gate(ad, Dd, gd, xs, ws, asum, dgate, B, HW, C)
        outs.append((xs.cpu(), asum.cpu(), dgate.cpu()))
    xs, asum, dgate = outs[0]
    a64, D64 = a.double(), D.double()
    assert torch.equal(xs.double(), a64 * g.double()[:, None]) and torch.equal(asum.double(), a64.sum(1))
    assert torch.equal(dgate.double(), (D64 * a64).sum(1))
    assert all(torch.equal(x, y) for x, y in zip(*outs)), "two runs differ"


def test_gate_backward_checks_its_arguments():
    B, HW, C = 2, 9, 8
    a, D, xs = (torch.zeros(B, HW, C, device=DEV) for _ in range(3))
    g, asum, dgate = (torch.full((B, C), 7.0, device=DEV) for _ in range(3))
    xs.fill_(7.0)
    ws = torch.full((capi.lib().stl_det_mbconv_gate_bwd_workspace(B, HW, C),), 7.0, device=DEV)
    for bad in range(7):
        args = [a, D, g, xs, ws, asum, dgate]
        args[bad] = None
        with pytest.raises(RuntimeError, match="det_mbconv_gate_bwd: null pointer"):
            _gate(*args, B, HW, C)
    for dims in ((0, HW, C), (B, 0, C), (B, HW, 0), (B, -1, C)):
        with pytest.raises(RuntimeError, match="det_mbconv_gate_bwd: B"):
            _gate(a, D, g, xs, ws, asum, dgate, *dims)
    with pytest.raises(RuntimeError, match="det_mbconv_gate_bwd: .* too large"):
        _gate(a, D, g, xs, ws, asum, dgate, 65536, HW, C)
    with pytest.raises(RuntimeError, match="det_mbconv_gate_bwd: xs overlaps"):
        _gate(a, D, g, a, ws, asum, dgate, B, HW, C)
    assert all(bool((t == 7.0).all()) for t in (xs, ws, asum, dgate)), "a refused call wrote something"
    assert capi.lib().stl_det_mbconv_gate_bwd_workspace(0, HW, C) == 0 and capi.lib().stl_det_mbconv_parts(0) == 0


# ------------------------------------------------------------------------------------------------ stl_det_se_bwd alone
def _se_ref(asum, dgate, w1, b1, w2, b2, HW, dtype):
    """The gate from the pooling sums and its backward given dL/dg = dgate, by autograd in `dtype` -> (g, dpool, dw1, db1, dw2, db2)."""
    p = (asum.to(dtype) / HW).requires_grad_(True)
    w1, b1, w2, b2 = (t.to(dtype).clone().requires_grad_(True) for t in (w1, b1, w2, b2))
    g = torch.sigmoid(torch.nn.functional.silu(p @ w1.t() + b1) @ w2.t() + b2)
    (g * dgate.to(dtype)).sum().backward()
    return g.detach(), p.grad, w1.grad, b1.grad, w2.grad, b2.grad


@pytest.mark.parametrize("B,C,Cs", [(1, 8, 1), (2, 1152, 48), (3, 1392, 58), (2, 2304, 96)])
def test_se_backward(B, C, Cs):
    HW = 256
    gen = torch.Generator().manual_seed(C + Cs)
    asum = torch.randn(B, C, generator=gen) * HW * 0.5
    dgate = torch.randn(B, C, generator=gen)
    w1, b1 = torch.randn(Cs, C, generator=gen) / C ** 0.5, torch.randn(Cs, generator=gen) * 0.1
    w2, b2 = torch.randn(C, Cs, generator=gen) / Cs ** 0.5, torch.randn(C, generator=gen) * 0.1
    y64 = _se_ref(asum, dgate, w1, b1, w2, b2, HW, torch.float64)
    y32 = _se_ref(asum, dgate, w1, b1, w2, b2, HW, torch.float32)
    dev = [t.to(DEV) for t in (asum, dgate, y64[0].float(), w1, b1, w2, b2)]   # the stored gate: the fp64 one rounded once
    outs = []
    for _ in range(2):
        ws = _nan(capi.lib().stl_det_se_bwd_workspace(B, C, Cs))
        o = [_nan(B, C), _nan(Cs, C), _nan(Cs), _nan(C, Cs), _nan(C)]
        capi.call("stl_det_se_bwd", *[t.data_ptr() for t in dev[:3]], B, HW, C, Cs, *[t.data_ptr() for t in dev[3:]], ws.data_ptr(),
                  *[t.data_ptr() for t in o], _st())
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in o])
    for name, got, a64, a32 in zip(("dpool", "dw1", "db1", "dw2", "db2"), outs[0], y64[1:], y32[1:]):
        _hold(f"se_bwd {B} {C} {Cs} {name}", got, a64, a32)
    assert all(torch.equal(x, y) for x, y in zip(*outs)), "two runs differ"


def test_se_backward_checks_its_arguments():
    B, HW, C, Cs = 2, 4, 8, 2
    t = [torch.full((n,), 0.5, device=DEV) for n in (B * C, B * C, B * C, Cs * C, Cs, C * Cs, C)]
    ws = torch.full((capi.lib().stl_det_se_bwd_workspace(B, C, Cs),), 7.0, device=DEV)
    o = [torch.full((n,), 7.0, device=DEV) for n in (B * C, Cs * C, Cs, C * Cs, C)]

    def run(t_, dims, ws_, o_):
        capi.call("stl_det_se_bwd", *[_ptr(x) for x in t_[:3]], *dims, *[_ptr(x) for x in t_[3:]], _ptr(ws_), *[_ptr(x) for x in o_], _st())
        torch.cuda.synchronize()
    for bad in range(7):
        with pytest.raises(RuntimeError, match="det_se_bwd: null pointer"):
            run(t[:bad] + [None] + t[bad + 1:], (B, HW, C, Cs), ws, o)
    for bad in range(5):
        with pytest.raises(RuntimeError, match="det_se_bwd: null pointer"):
            run(t, (B, HW, C, Cs), ws, o[:bad] + [None] + o[bad + 1:])
    with pytest.raises(RuntimeError, match="det_se_bwd: null pointer"):
        run(t, (B, HW, C, Cs), None, o)
    for dims in ((0, HW, C, Cs), (B, 0, C, Cs), (B, HW, 0, Cs), (B, HW, C, 0)):
        with pytest.raises(RuntimeError, match="det_se_bwd: B"):
            run(t, dims, ws, o)
    with pytest.raises(RuntimeError, match="det_se_bwd: .* above 8192"):
        run(t, (B, HW, 8190, 3), ws, o)
    with pytest.raises(RuntimeError, match="det_se_bwd: B 65536 too large"):
        run(t, (65536, HW, C, Cs), ws, o)
    assert all(bool((x == 7.0).all()) for x in [ws] + o), "a refused call wrote something"
    assert capi.lib().stl_det_se_bwd_workspace(B, C, 0) == 0


# ------------------------------------------------------------------------------------------------ stl_det_mbconv_act_bwd alone
def _act(D, u, g, dpool, du, ws, db, B, HW, C):
    capi.call("stl_det_mbconv_act_bwd", _ptr(D), _ptr(u), _ptr(g), _ptr(dpool), _ptr(du), _ptr(ws), _ptr(db), B, HW, C, _st())
    torch.cuda.synchronize()


def _act_ref(D, u, g, dpool, HW, dtype):
    D, u, g, dpool = (t.to(dtype) for t in (D, u, g, dpool))
    s = torch.sigmoid(u)
    du = (D * g[:, None] + dpool[:, None] / HW) * (s * (1 + u * (1 - s)))
    return du, du.sum((0, 1))


@pytest.mark.parametrize("B,HW,C", GATE_SHAPES)
def test_act_backward(B, HW, C):
    lib = capi.lib()
    if (B, HW, C) == GATE_SHAPES[-1]:
        assert lib.stl_det_mbconv_act_bwd_parts(B, HW) > 1, "the bias sum must cross more than one partial"
    assert lib.stl_det_mbconv_act_bwd_parts(B, HW) == B * lib.stl_det_mbconv_parts(HW)
    gen = torch.Generator().manual_seed(HW * 3 + C)
    D, u = torch.randn(B, HW, C, generator=gen), torch.randn(B, HW, C, generator=gen) * 2
    g, dpool = torch.rand(B, C, generator=gen), torch.randn(B, C, generator=gen) * HW
    (du64, db64), (du32, db32) = _act_ref(D, u, g, dpool, HW, torch.float64), _act_ref(D, u, g, dpool, HW, torch.float32)
    Dd, ud, gd, pd = (t.to(DEV) for t in (D, u, g, dpool))
    outs = []
    for inplace in (False, False, True):   # twice apart, then du = D
        du = Dd.clone() if inplace else _nan(B, HW, C)
        db, ws = _nan(C), _nan(lib.stl_det_mbconv_act_bwd_workspace(B, HW, C))
        _act(du if inplace else Dd, ud, gd, pd, du, ws, db, B, HW, C)
        outs.append((du.cpu(), db.cpu()))
    _hold(f"act_bwd {B} {HW} {C} du", outs[0][0], du64, du32)
    _hold(f"act_bwd {B} {HW} {C} db", outs[0][1], db64, db32)
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1])), "two runs differ"
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[2])), "du = D gives other bits"


def test_act_backward_checks_its_arguments():
    B, HW, C = 2, 9, 8
    D, u = torch.zeros(B, HW, C, device=DEV), torch.zeros(B, HW, C, device=DEV)
    g, dpool = torch.zeros(B, C, device=DEV), torch.zeros(B, C, device=DEV)
    du, db = torch.full((B, HW, C), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
    ws = torch.full((capi.lib().stl_det_mbconv_act_bwd_workspace(B, HW, C),), 7.0, device=DEV)
    for bad in range(7):
        args = [D, u, g, dpool, du, ws, db]
        args[bad] = None
        with pytest.raises(RuntimeError, match="det_mbconv_act_bwd: null pointer"):
            _act(*args, B, HW, C)
    for dims in ((0, HW, C), (B, 0, C), (B, HW, 0)):
        with pytest.raises(RuntimeError, match="det_mbconv_act_bwd: B"):
            _act(D, u, g, dpool, du, ws, db, *dims)
    with pytest.raises(RuntimeError, match="det_mbconv_act_bwd: .* too large"):
        _act(D, u, g, dpool, du, ws, db, 65536, HW, C)
    with pytest.raises(RuntimeError, match="det_mbconv_act_bwd: du overlaps u"):
        _act(D, du, g, dpool, du, ws, db, B, HW, C)
    both = torch.full((2 * B * HW * C,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="det_mbconv_act_bwd: du overlaps D without being D"):
        _act(both[4:], u, g, dpool, both, ws, db, B, HW, C)
    assert all(bool((t == 7.0).all()) for t in (du, ws, db, both)), "a refused call wrote something"
    assert capi.lib().stl_det_mbconv_act_bwd_workspace(B, 0, C) == 0 and capi.lib().stl_det_mbconv_act_bwd_parts(0, HW) == 0


# ------------------------------------------------------------------------------------------------ the whole method
GATED = ("expand", "expand_bn", "depthwise", "depthwise_bn", "se")   # the classes the gate's path reaches


def _run(cc, kbs):
    """One model with every BiFPN cell training; per kb in kbs one detection_loss + backward on the same input with
    set_train_backbone(kb), and the plan's maps the yardstick starts from and routes by (the forward does not depend on kb)."""
    m, sd = _model(cc)
    targets = TARGETS[cc]
    chw = [torch.from_numpy(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255)) for im in R.images()[:len(targets)]]
    o = dict(m=m, sd=sd, chw=chw, targets=targets, runs={})
    o["plan"] = plan = m.plan(len(chw), DEV)
    o["buffers"] = {k: v.clone() for k, v in m.named_buffers()}
    m.set_train_bifpn("all")
    for kb in kbs:
        m.set_train_backbone(kb)
        for q in m.parameters():
            q.grad = None
        loss = m.detection_loss(chw, targets)
        assert m.plan(len(chw), DEV) is plan
        tr = plan.train
        sum(loss.values()).backward()
        torch.cuda.synchronize()
        o["runs"][kb] = dict(loss={n: v.detach().clone() for n, v in loss.items()}, reg=tr.reg.clone(), cls=tr.cls.clone(),
                             grads={n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None},
                             want=[n for n, _ in T.trainable_parameters(m)])
    assert all(torch.equal(v, o["buffers"][k]) for k, v in m.named_buffers()), "a buffer changed"
    o["levels"] = [[_nchw(kept[n][2]) for n in LEVEL_NODES] for kept in plan.cells]
    o["p34"] = [_nchw(f) for f in plan.backbone[:2]]
    o["t"], o["p6"] = _nchw(plan.first_pools[0][1]), _nchw(plan.first_pools[0][2])
    o["inputs"] = [_nchw(rec[0]) for rec in plan.blocks]   # every block's stored input
    gt, offsets = T.pack_targets(targets, [tuple(c.shape[1:]) for c in chw], 1)
    o["loss_args"] = (torch.from_numpy(m.anchors_np), torch.from_numpy(gt), offsets.tolist())
    return o


def _check_blocks(o, cc, kb, tag):
    """Every block gradient of the run with kb trainable blocks against the yardstick run from the first trainable block's stored
    input, every pool routed by the stored map; and against the variant with the gate held constant, which the device must NOT match."""
    n, nb = len(o["levels"]), len(o["inputs"])
    blocks = list(range(nb - kb, nb))
    routes = {j: dict(zip(BR.POOLED, o["levels"][j][:4])) for j in range(n)}
    routes[0].update(t=o["t"], p6=o["p6"])
    args = (o["sd"], cc, 1, n, blocks, o["inputs"][blocks[0]], o["p34"], routes, *o["loss_args"])
    c64, r64, g64 = KR.method_yardstick(*args, torch.float64)
    c32, r32, g32 = KR.method_yardstick(*args, torch.float32)
    _, _, gcut = KR.method_yardstick(*args, torch.float64, detach_gate=True)
    run = o["runs"][kb]
    _hold(f"{tag} classification", run["loss"]["classification"], c64, c32)
    _hold(f"{tag} regression", run["loss"]["regression"], r64, r32)
    assert set(run["grads"]) == set(run["want"]) == set(g64), "a gradient outside trainable_parameters, or one missing"
    mine = [name for name in run["want"] if name.startswith("backbone_net.")]
    assert len(mine) == 13 * kb and all(name.startswith(tuple(f"{KR.PRE}{i}." for i in blocks)) for name in mine)
    for name, q in o["m"].named_parameters():
        if name.startswith("backbone_net.") and name not in mine:
            assert q.grad is None and name not in run["grads"], name
    for name in mine:
        got, cls = run["grads"][name], KR.tensor_class(name)
        assert got.shape == g64[name].shape and bool(got.abs().max() > 0), name
        _hold(f"{tag} {name}", got, g64[name], g32[name], cls)
        if cls in GATED:   # the test sees a missing gate path
            # on the yardstick's own scale, as e is (the variant's SE gradients are zero)
            gap = (got.cpu().double() - gcut[name]).abs().max().item() / g64[name].abs().max().item()
            print(f"{tag} {name}: against the constant-gate variant {gap:.3e}")
            assert gap > _bound(g32[name], g64[name]), (name, gap)
    print(f"{tag} ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


def _check_bitwise_behind(o, kb):
    """Losses, reg, cls and every BiFPN / head gradient of the run with kb blocks are those of kb = 0 bit for bit."""
    base, run = o["runs"][0], o["runs"][kb]
    assert all(torch.equal(run["loss"][n], base["loss"][n]) for n in ("classification", "regression"))
    assert torch.equal(run["reg"], base["reg"]) and torch.equal(run["cls"], base["cls"])
    assert set(base["grads"]) == {n for n in run["grads"] if not n.startswith("backbone_net.")} and len(base["grads"]) > 100
    assert all(n.startswith(("bifpn.", "regressor.", "classifier.")) for n in base["grads"])
    for n, g in base["grads"].items():
        assert torch.equal(run["grads"][n], g), n


@pytest.fixture(scope="module")
def d0():
    return _run(0, (0, 1))


def test_d0_block_gradients_match_the_yardstick_and_nothing_behind_moves(d0):
    assert d0["m"].train_backbone == 1 and d0["m"].train_bifpn == 3
    _check_bitwise_behind(d0, 1)
    assert d0["inputs"][15].shape[1:] == (192, 16, 16) and d0["plan"].blocks[15][2].shape[3] == 1152
    _check_blocks(d0, 0, 1, "d0 k1")


def test_d0_two_runs_are_bitwise_equal(d0):
    m = d0["m"]
    assert m.train_backbone == 1
    for q in m.parameters():
        q.grad = None
    loss = m.detection_loss(d0["chw"], d0["targets"])
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    first = d0["runs"][1]
    assert all(torch.equal(loss[n], first["loss"][n]) for n in loss)
    assert {n for n, q in m.named_parameters() if q.grad is not None} == set(first["grads"])
    for n, g in first["grads"].items():
        assert torch.equal(dict(m.named_parameters())[n].grad, g), n


def test_d3_both_blocks_train_through_the_expand_layer_and_the_skip():
    """mid 1392 / 2304, se 58 / 96; block 25 has the identity skip, so block 24's gradients hold the expand layer's data gradient and
    dy itself.  k = 1 on the same model leaves block 24 alone."""
    o = _run(3, (0, 1, 2))
    specs = E.block_specs(3)
    assert [b["mid"] for b in specs[24:]] == [1392, 2304] and [b["skip"] for b in specs[24:]] == [False, True]
    assert not any(n.startswith(f"{KR.PRE}24.") for n in o["runs"][1]["grads"])
    assert sum(n.startswith(f"{KR.PRE}25.") for n in o["runs"][1]["grads"]) == 13
    _check_bitwise_behind(o, 2)
    _check_bitwise_behind(o, 1)
    for n, g in o["runs"][1]["grads"].items():   # block 25's do not depend on whether block 24 trains
        assert torch.equal(o["runs"][2]["grads"][n], g), n
    _check_blocks(o, 3, 2, "d3 k2")


def test_sgd_step_keeps_the_plan_and_refolds_from_the_first_trainable_block_exactly(d0):
    m, plan = d0["m"], d0["plan"]
    m.set_train_bifpn("all").set_train_backbone(1)
    loss = m.detection_loss(d0["chw"], d0["targets"])
    sum(loss.values()).backward()
    wbuf, before = m._wbuf, m._wbuf.clone()
    params = [q for _, q in T.trainable_parameters(m)]
    assert all(q.grad is not None for q in params)
    torch.optim.SGD(params, lr=1e-3).step()
    assert m.plan(len(d0["chw"]), DEV) is plan and m._wbuf is wbuf and plan.train is not None
    fresh = E.setup_detector("efficientdet", "d0")
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.to(DEV).ready(DEV)
    first, cells = m._block_off[15][0], m._tail_off[0][0]
    assert 0 < m._block_off[14][0] < first < cells
    assert torch.equal(m._wbuf, fresh._wbuf) and torch.equal(m._wbuf[:first], before[:first])
    lay = m._layout["blocks"][15]
    ends = sorted([lay["dw"][1], lay["dw"][0], lay["project"][1], lay["project"][0], lay["expand"][1], lay["expand"][0], *lay["se"], cells])
    assert ends[0] == first
    for lo, hi in zip(ends[:-1], ends[1:]):   # every piece of the block moved: both biases, the three weights, the four SE arrays
        assert not torch.equal(m._wbuf[lo:hi], before[lo:hi]), lo
    again = m.detection_loss(d0["chw"], d0["targets"])
    sum(again.values()).backward()
    assert all(bool(torch.isfinite(v)) for v in again.values())
    assert not torch.equal(again["classification"], d0["runs"][0]["loss"]["classification"])   # the step moved the network
    assert not torch.equal(again["regression"], d0["runs"][0]["loss"]["regression"])


def test_loss_weights_reach_the_blocks():
    """The blocks' gradients are linear in the two losses' gradients: 2 * classification + 0.5 * regression."""
    m, _ = _model(0)
    m.set_train_bifpn("all").set_train_backbone(1)
    targets = TARGETS[0]
    chw = [torch.from_numpy(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255)) for im in R.images()[:len(targets)]]
    grads = {}
    for tag, (wc, wr) in (("c", (1.0, 0.0)), ("r", (0.0, 1.0)), ("mix", (2.0, 0.5))):
        for q in m.parameters():
            q.grad = None
        loss = m.detection_loss(chw, targets)
        (wc * loss["classification"] + wr * loss["regression"]).backward()
        grads[tag] = {n: q.grad.clone() for n, q in T.trainable_parameters(m) if n.startswith("backbone_net.")}
    assert len(grads["mix"]) == 13
    for n, g in grads["mix"].items():
        want = 2.0 * grads["c"][n].double() + 0.5 * grads["r"][n].double()
        assert bool(want.abs().max() > 0) and (g.double() - want).abs().max() <= 1e-4 * want.abs().max() + 1e-12, n


# ------------------------------------------------------------------------------------------------ DetectorTrainer
def test_detector_trainer_trains_the_last_block_and_resumes(tmp_path):
    from stlpose_amd.det_data import DetBatchLoader
    from stlpose_amd.detector_trainer import DetectorTrainer
    from stlpose_amd.pose_data import ResidentImages
    from tests import test_det_batch_gpu as DB
    images, db = DB._images(DB.T_SIZES, 21), DB._db(DB.T_SIZES, DB.T_BOXES, DB.T_LABELS)
    store = ResidentImages.from_arrays(images, DEV)

    def trainer(exp_path, **kw):
        exp = DB._exp_data()
        exp["training"]["train_bifpn"] = "all"
        exp["training"]["train_backbone"] = 1
        model = DB._model(train_header=True)
        train, valid = DetBatchLoader(db, store, exp, 2, True, seed=3), DetBatchLoader(db, store, exp, 2, False)
        return DetectorTrainer(str(exp_path), exp, model, train, valid, db.coco_gt(256), valid_fraction=1.0, **kw)
    t = trainer(tmp_path / "full")
    assert t.model.train_bifpn == 3 and t.model.train_backbone == 1
    optimised = {id(q) for group in t.optimizer.param_groups for q in group["params"]}
    assert optimised == {id(q) for _, q in T.trainable_parameters(t.model)}
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    t.training_loop()
    logs = json.loads((tmp_path / "full" / "detector_logs.json").read_text())
    assert len(logs["train_loss"]) == 2 and t.skipped == 0 and all(np.isfinite(logs["train_loss"]))
    after = t.model.state_dict()
    params = {n for n, _ in t.model.named_parameters()}
    last = len(t.model.backbone_net.model._blocks) - 1
    for k, v in after.items():
        if k.startswith((f"{KR.PRE}{last}.", "bifpn.")) and k in params:
            assert not torch.equal(v, before[k]), k          # the last block trains, every parameter of it
        elif not k.startswith(("regressor.", "classifier.")):
            assert torch.equal(v, before[k]), k              # the blocks in front, the stem, every buffer
    saved = tmp_path / "full" / "models" / "detector"
    os.makedirs(tmp_path / "resumed")
    shutil.copy(tmp_path / "full" / "detector_logs.json", tmp_path / "resumed" / "detector_logs.json")
    r = trainer(tmp_path / "resumed", checkpoint=str(saved / "checkpoint_epoch_0.pth"), resume_training=True)
    assert r.cur_epoch == 1 and r.model.train_backbone == 1
    r.training_loop()
    for k, v in after.items():
        assert torch.equal(v, r.model.state_dict()[k]), k
