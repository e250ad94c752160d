"""GPU: training the first BiFPN cell with the others and the heads (``set_train_bifpn("all")``; csrc/detector_bifpn.hip,
stlpose_amd/detector_train.py) against the fp64 yardstick tests/detector_bifpn_first_ref.py: stl_det_pool_bwd alone (exact),
EfficientDetBackbone.detection_loss end to end (D0 on the two test images, D3 on one), the optimiser step's refold from cell 0,
linearity in the two losses and DetectorTrainer.

Bounds: the rule of tests/test_detector_train_gpu.py and tests/test_detector_bifpn_gpu.py.  Each figure is e = max|device - Y| /
max|Y| of one tensor against the fp64 yardstick Y and is held to max(MARGIN * e32, FLOOR), e32 being the same figure of the fp32
torch evaluation of the same yardstick with the same pool routing (the device's own stored fp32 maps), MARGIN = 8, FLOOR = 1e-6.  The
measured ratios per tensor class are in DESIGN.md ("Training the first BiFPN cell")."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, detector_train as T, efficientdet as E
from tests import detector_bifpn_first_ref as FR, detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR
from tests.test_detector_train_gpu import TARGETS, _model

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 8.0
RATIOS = {}   # tensor class -> the largest e / e32 among its figures above the floor, printed by the tests that fill it


def _st():
    return torch.cuda.current_stream().cuda_stream


def _hold(name, got, y64, y32, cls=None):
    """Print the figures, then hold e to max(MARGIN * e32, FLOOR)."""
    e, e32 = TR.rel_err(got, y64), TR.rel_err(y32, y64)
    ratio = e / e32 if e32 else float("inf") if e else 0.0
    print(f"{name}: e {e:.3e} e32 {e32:.3e} ratio {ratio:.2f}")
    if cls is not None and e > TR.FLOOR:
        RATIOS[cls] = max(RATIOS.get(cls, 0.0), ratio)
    assert e <= max(MARGIN * e32, TR.FLOOR), (name, e, e32)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------ stl_det_pool_bwd alone
class _PoolBwd:
    """One case: an S x S map of small integers (negatives included: exact ties everywhere, border windows won by the padding) pooled
    into ceil(S / 2), an integer-valued dy, and the fp64 autograd of routed_pool -- every sum of up to four terms is exact."""

    def __init__(self, S, Cn, B=2):
        g = torch.Generator().manual_seed(100 * S + Cn)
        self.S, self.H = S, (S + 1) // 2
        self.x = torch.randint(-2, 3, (B, Cn, S, S), generator=g).float()
        self.dy = torch.randint(-3, 4, (B, Cn, self.H, self.H), generator=g).float()
        self.base = torch.randint(-5, 6, (B, Cn, S, S), generator=g).float()
        x64 = self.x.double().requires_grad_(True)
        (BR.routed_pool(x64, self.x) * self.dy.double()).sum().backward()
        self.dx64 = x64.grad
        self.xd, self.dyd = _nhwc(self.x), _nhwc(self.dy)
        f = self.f = capi.DetFuse()
        f.B, f.H, f.W, f.C, f.nterms = B, self.H, self.H, Cn, 1
        f.t[0] = capi.DetTerm(self.xd.data_ptr(), 2, S, S, 0)
        f.wparam, f.out = None, None

    def run(self, dx, accumulate=0, dy=None):
        capi.call("stl_det_pool_bwd", C.byref(self.f), (self.dyd if dy is None else dy).data_ptr(), None if dx is None else dx.data_ptr(),
                  accumulate, _st())
        torch.cuda.synchronize()
        return dx


@pytest.mark.parametrize("Cn", [8, 160, 6])   # 8 and 160: four channels per thread; 6: the scalar path
@pytest.mark.parametrize("S", [5, 6, 8])      # pads 1 / 1, 0 / 1, 0 / 1
def test_pool_backward_is_exact(S, Cn):
    p = _PoolBwd(S, Cn)
    # what the case rests on, read off the yardstick's side: exact ties, and windows the padding wins
    padded = R._same(p.x, 3, 2)
    top, idx = F.max_pool2d(padded, 3, 2, return_indices=True)
    cols = F.unfold(padded, 3, stride=2).view(p.x.shape[0], p.x.shape[1], 9, -1)
    assert ((cols == top.flatten(2)[:, :, None]).sum(2) > 1).any(), "no exact tie"
    py = (padded.shape[2] - S) // 2
    iy, ix = idx // padded.shape[3] - py, idx % padded.shape[3] - py
    lost = (iy < 0) | (iy >= S) | (ix < 0) | (ix >= S)
    assert lost.any(), "no window won by the padding"
    assert p.dx64.sum() == (p.dy.double() * ~lost).sum(), "a window won by a padded tap gives its gradient to nobody"
    want = p.dx64.permute(0, 2, 3, 1).float()
    dx = p.run(torch.full_like(p.xd, float("nan")))
    assert torch.equal(dx.cpu(), want)
    assert torch.equal(p.run(torch.full_like(p.xd, float("nan"))), dx), "two runs differ"
    base = _nhwc(p.base)
    acc = p.run(base.clone(), accumulate=1)
    assert torch.equal(acc.cpu(), (p.base.double() + p.dx64).permute(0, 2, 3, 1).float())
    assert torch.equal(p.run(base.clone(), accumulate=1), acc), "two accumulating runs differ"


def test_pool_backward_checks_its_arguments():
    p = _PoolBwd(6, 8)
    dx = torch.zeros_like(p.xd)
    p.run(dx)   # the descriptor is good as it stands
    w = torch.ones(1, device=DEV)
    p.f.wparam = w.data_ptr()   # a weighted node is stl_det_fuse_bwd's
    with pytest.raises(RuntimeError, match="det_pool_bwd"):
        p.run(dx)
    p.f.wparam = None
    p.f.t[0].mode = 0
    with pytest.raises(RuntimeError, match="det_pool_bwd: term mode 0"):
        p.run(dx)
    p.f.t[0].mode = 2
    p.f.nterms = 2
    with pytest.raises(RuntimeError, match="det_pool_bwd: 2 terms"):
        p.run(dx)
    p.f.nterms = 1
    p.f.t[0].H = 7   # 7 x 6 does not pool into 3 x 3
    with pytest.raises(RuntimeError, match="det_pool_bwd: term mode 2 of 7 x 6"):
        p.run(dx)
    p.f.t[0].H = 6
    with pytest.raises(RuntimeError, match="det_pool_bwd: null pointer"):
        p.run(None)
    both = torch.zeros(p.xd.numel() + p.dyd.numel(), device=DEV)
    for dy in (both, both[p.xd.numel() - 4:]):   # dx = both[:numel of x]: dy at its start, and dy's first floats on its last ones
        with pytest.raises(RuntimeError, match="det_pool_bwd: dy and dx overlap"):
            p.run(both, dy=dy)
    p.run(both, dy=both[p.xd.numel():])   # side by side is no overlap
    assert torch.equal(p.run(torch.empty_like(p.xd)), dx)


# ------------------------------------------------------------------------------------------------ the whole method
LEVEL_NODES = ("conv3_up", "conv4_down", "conv5_down", "conv6_down", "conv7_down")   # the nodes whose outputs are a cell's five levels


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).float().cpu()


def _run(cc, ks):
    """One model; per k in ks (an integer or "all") one detection_loss + backward on the same input, and the plan's maps the
    yardstick starts from and routes by (the forward does not depend on k)."""
    m, sd = _model(cc)
    targets = TARGETS[cc]
    chw = [torch.from_numpy(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255)) for im in R.images()[:len(targets)]]
    o = dict(m=m, sd=sd, chw=chw, targets=targets, runs={})
    o["plan"] = plan = m.plan(len(chw), DEV)
    for k in ks:
        m.set_train_bifpn(k)
        for q in m.parameters():
            q.grad = None
        loss = m.detection_loss(chw, targets)
        assert m.plan(len(chw), DEV) is plan
        tr = plan.train
        sum(loss.values()).backward()
        torch.cuda.synchronize()
        o["runs"][k] = dict(loss={n: v.detach().clone() for n, v in loss.items()}, reg=tr.reg.clone(), cls=tr.cls.clone(),
                            grads={n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None})
    o["levels"] = [[_nchw(kept[n][2]) for n in LEVEL_NODES] for kept in plan.cells]   # per cell its five outputs as the device stored them
    o["p345"] = [_nchw(f) for f in plan.backbone]
    o["t"], o["p6"] = _nchw(plan.first_pools[0][1]), _nchw(plan.first_pools[0][2])
    assert plan.first_pools[1][1] is plan.first_pools[0][2] and plan.first_convs["p5_to_p6"][1] is plan.first_pools[0][1]
    gt, offsets = T.pack_targets(targets, [tuple(c.shape[1:]) for c in chw], 1)
    o["loss_args"] = (torch.from_numpy(m.anchors_np), torch.from_numpy(gt), offsets.tolist())
    return o


def _check_first_cell(o, cc, tag):
    """Every gradient of the "all" run against the yardstick run from the backbone's stored P3 / P4 / P5, every pool routed by the
    stored map; the first cell's are held here (the other cells' and the heads': bitwise those of k = cells - 1, by the caller)."""
    n = len(o["levels"])
    routes = {j: dict(zip(BR.POOLED, o["levels"][j][:4])) for j in range(n)}
    routes[0].update(t=o["t"], p6=o["p6"])
    args = (o["sd"], cc, 1, n, o["p345"], routes, *o["loss_args"])
    (c64, r64, g64), (c32, r32, g32) = FR.method_yardstick(*args, torch.float64), FR.method_yardstick(*args, torch.float32)
    run = o["runs"]["all"]
    _hold(f"{tag} classification", run["loss"]["classification"], c64, c32)
    _hold(f"{tag} regression", run["loss"]["regression"], r64, r32)
    want = {name for name, _ in T.trainable_parameters(o["m"].set_train_bifpn("all"))}
    assert set(run["grads"]) == want == set(g64), "a gradient outside trainable_parameters, or one missing"
    assert not any(name.startswith("backbone_net.") for name in run["grads"])
    assert all(q.grad is None for q in o["m"].backbone_net.parameters())
    first = sorted(name for name in g64 if name.startswith("bifpn.0."))
    assert len(first) == 8 + 8 * 5 + 24
    for name in first:
        assert run["grads"][name].shape == g64[name].shape, name
        _hold(f"{tag} {name}", run["grads"][name], g64[name], g32[name], FR.tensor_class(name))
    print(f"{tag} ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


@pytest.fixture(scope="module")
def d0():
    return _run(0, (0, 2, "all"))


def test_d0_all_is_bitwise_the_trailing_cells_and_the_first_cell_matches_the_yardstick(d0):
    base, tail, run = d0["runs"][0], d0["runs"][2], d0["runs"]["all"]
    assert d0["m"].train_bifpn == len(d0["m"].bifpn) == 3
    assert all(torch.equal(run["loss"][n], base["loss"][n]) for n in ("classification", "regression"))
    assert torch.equal(run["reg"], base["reg"]) and torch.equal(run["cls"], base["cls"])
    assert set(tail["grads"]) == {n for n in run["grads"] if not n.startswith("bifpn.0.")}
    for n, g in tail["grads"].items():   # the heads' and cells 1 and 2's run through the same launches
        assert torch.equal(run["grads"][n], g), n
    _check_first_cell(d0, 0, "d0 all")


def test_d3_first_cell_gradients_match_the_yardstick():
    """C = 160 and Ci = 48 / 136 / 384 are no multiples of the 64-wide tile; batch 1."""
    o = _run(3, ("all",))
    assert o["m"].train_bifpn == 6 and [f.shape[1] for f in o["p345"]] == [48, 136, 384]
    _check_first_cell(o, 3, "d3 all")


def test_sgd_step_keeps_the_plan_and_refolds_from_the_first_cell_exactly(d0):
    m, plan = d0["m"], d0["plan"]
    m.set_train_bifpn("all")
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
    first = m._tail_off[0][0]
    assert 0 < first < m._tail_off[1][0]
    assert torch.equal(m._wbuf, fresh._wbuf) and torch.equal(m._wbuf[:first], before[:first])
    assert not torch.equal(m._wbuf[first:m._tail_off[1][0]], before[first:m._tail_off[1][0]])   # the first cell's pieces moved
    again = m.detection_loss(d0["chw"], d0["targets"])
    sum(again.values()).backward()
    assert all(bool(torch.isfinite(v)) for v in again.values())
    assert not torch.equal(again["classification"], d0["runs"][0]["loss"]["classification"])   # the step moved the network
    assert not torch.equal(again["regression"], d0["runs"][0]["loss"]["regression"])


def test_loss_weights_reach_the_first_cell(d0):
    """The cells' gradients are linear in the two losses' gradients: 2 * classification + 0.5 * regression."""
    m = d0["m"]
    m.set_train_bifpn("all")
    grads = {}
    for tag, (wc, wr) in (("c", (1.0, 0.0)), ("r", (0.0, 1.0)), ("mix", (2.0, 0.5))):
        for q in m.parameters():
            q.grad = None
        loss = m.detection_loss(d0["chw"], d0["targets"])
        (wc * loss["classification"] + wr * loss["regression"]).backward()
        grads[tag] = {n: q.grad.clone() for n, q in T.trainable_parameters(m) if n.startswith("bifpn.0.")}
    assert len(grads["mix"]) == 8 + 8 * 5 + 24
    for n, g in grads["mix"].items():
        want = 2.0 * grads["c"][n].double() + 0.5 * grads["r"][n].double()
        assert (g.double() - want).abs().max() <= 1e-4 * want.abs().max() + 1e-12, n


# ------------------------------------------------------------------------------------------------ DetectorTrainer
def test_detector_trainer_trains_every_cell_and_resumes(tmp_path):
    from stlpose_amd.det_data import DetBatchLoader
    from stlpose_amd.detector_trainer import DetectorTrainer
    from stlpose_amd.pose_data import ResidentImages
    from tests import test_det_batch_gpu as DB
    images, db = DB._images(DB.T_SIZES, 21), DB._db(DB.T_SIZES, DB.T_BOXES, DB.T_LABELS)
    store = ResidentImages.from_arrays(images, DEV)

    def trainer(exp_path, **kw):
        exp = DB._exp_data()
        exp["training"]["train_bifpn"] = "all"
        model = DB._model(train_header=True)
        train, valid = DetBatchLoader(db, store, exp, 2, True, seed=3), DetBatchLoader(db, store, exp, 2, False)
        return DetectorTrainer(str(exp_path), exp, model, train, valid, db.coco_gt(256), valid_fraction=1.0, **kw)
    t = trainer(tmp_path / "full")
    assert t.model.train_bifpn == 3
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    t.training_loop()
    logs = json.loads((tmp_path / "full" / "detector_logs.json").read_text())
    assert sorted(logs) == ["last_modified", "train_loss", "valid_ap"] and len(logs["train_loss"]) == 2 and t.skipped == 0
    assert all(np.isfinite(logs["train_loss"]))
    after = t.model.state_dict()
    params = {n for n, _ in t.model.named_parameters()}
    for k, v in after.items():
        if k.startswith("bifpn.") and k in params:
            assert not torch.equal(v, before[k]), k          # every cell trains, every parameter of it
        elif not k.startswith(("regressor.", "classifier.")):
            assert torch.equal(v, before[k]), k              # the backbone, every buffer
    saved = tmp_path / "full" / "models" / "detector"
    ck = torch.load(saved / "checkpoint_epoch_final.pth", weights_only=False)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"] and ck["epoch"] == 2
    os.makedirs(tmp_path / "resumed")
    shutil.copy(tmp_path / "full" / "detector_logs.json", tmp_path / "resumed" / "detector_logs.json")
    r = trainer(tmp_path / "resumed", checkpoint=str(saved / "checkpoint_epoch_0.pth"), resume_training=True)
    assert r.cur_epoch == 1 and r.model.train_bifpn == 3
    r.training_loop()
    for k, v in after.items():
        assert torch.equal(v, r.model.state_dict()[k]), k
