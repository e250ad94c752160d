"""GPU: fine-tuning the trailing BiFPN cells with the heads (csrc/detector_bifpn.hip, stlpose_amd/detector_train.py) against the
fp64 yardstick tests/detector_bifpn_ref.py: stl_det_fuse_bwd and stl_det_grad_add alone, EfficientDetBackbone.detection_loss with
train_bifpn = k end to end (D0 on the two test images at k = 1 and 2, D3 at k = 1), the optimiser step's tail refold, the errors
and DetectorTrainer.

Bounds: the rule of tests/test_detector_train_gpu.py.  Each figure is e = max|device - Y| / max|Y| of one tensor against the fp64
yardstick Y and is held to max(MARGIN * e32, FLOOR), e32 being the same figure of the fp32 torch evaluation of the same yardstick
with the same pool routing (the device's own stored fp32 maps: see the yardstick's docstring), MARGIN = 8, FLOOR = 1e-6.  The
measured ratios per tensor class are in DESIGN.md ("Fine-tuning the trailing BiFPN cells")."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, detector_train as T, efficientdet as E
from tests import detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR
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


# ------------------------------------------------------------------------------------------------ stl_det_fuse_bwd alone
# (kind, S): "up" same + up into S x S from ceil(S / 2); "pool3" same + same + pool and "pool2" same + pool from S x S into
# ceil(S / 2): 5 pads 1 / 1, 6 and 8 pad 0 / 1
FUSE_CASES = [("up", 6), ("up", 5), ("pool3", 5), ("pool3", 6), ("pool3", 8), ("pool2", 5), ("pool2", 6), ("pool2", 8)]


def _fuse_case(kind, S, C, B=2, seed=0):
    """-> (terms [(fp32 NCHW map, mode)], raw weights p, dy NCHW, (H, W)).  Planted in a pooled map: channel 0 of image 0 all
    negative (the padding wins every window it is in: their gradient is dropped), an exact tie in image 1 between two neighbours
    of one row that lie in the same windows (columns 1, 2 under padding 1 / 1, columns 0, 1 under 0 / 1: the first wins them
    all).  C = 8 has a parameter <= 0."""
    g = torch.Generator().manual_seed(1000 * S + C + seed)
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    if kind == "up":
        H, small = S, (S + 1) // 2
        terms = [(r(B, C, H, H), 0), (r(B, C, small, small), 1)]
        p = torch.tensor([0.0, 0.9] if C == 8 else [0.6, 1.4])
    else:
        H = (S + 1) // 2
        x = r(B, C, S, S)
        x[0, 0] = -x[0, 0].abs() - 0.1
        x[1, 1, 1, S % 2] = x[1, 1, 1, S % 2 + 1] = 9.0
        terms = [(r(B, C, H, H), 0)] + ([(r(B, C, H, H), 0)] if kind == "pool3" else []) + [(x, 2)]
        p = torch.tensor(([1.2, -0.3, 0.8] if C == 8 else [0.5, 1.1, 0.9]) if kind == "pool3" else ([0.7, 1.3] if C == 8 else [1.6, 0.4]))
    return terms, p, r(B, C, H, H), (H, H)


def _fuse_yardstick(terms, p, dy, hw, dtype):
    """Autograd through swish(sum w^_i read_i) on the same fp32 inputs in `dtype` -> ([dx NHWC], dw^)."""
    ts = [t.to(dtype).requires_grad_(True) for t, _ in terms]
    what = BR.fusion_weights(p.to(dtype))
    what.requires_grad_(True)
    reads = [t if mode == 0 else BR.up(t, *hw) if mode == 1 else BR.routed_pool(t, src) for t, (src, mode) in zip(ts, terms)]
    out = torch.nn.functional.silu(sum(what[i] * x for i, x in enumerate(reads)))
    (out * dy.to(dtype)).sum().backward()
    return [t.grad.permute(0, 2, 3, 1) for t in ts], what.grad


class _FuseBwd:
    """The device side of one case: the descriptor, and runs with chosen destinations."""

    def __init__(self, terms, p, dy, hw):
        self.maps = [_nhwc(t) for t, _ in terms]
        self.p, self.dy = p.to(DEV), _nhwc(dy)
        B, C = dy.shape[:2]
        f = self.f = capi.DetFuse()
        f.B, f.H, f.W, f.C, f.nterms = B, hw[0], hw[1], C, len(terms)
        for i, (x, (_, mode)) in enumerate(zip(self.maps, terms)):
            f.t[i] = capi.DetTerm(x.data_ptr(), mode, x.shape[1], x.shape[2], 0)
        f.wparam = self.p.data_ptr()
        self.ws = torch.empty(capi.lib().stl_det_fuse_bwd_workspace(self.dy.numel()), device=DEV)

    def run(self, dst, accumulate=0):
        """dst: per term a tensor or None -> dw^ [nterms] (the dst are written in place)."""
        fb = capi.DetFuseBwd()
        for i, d in enumerate(dst):
            if d is not None:
                fb.dx[i], fb.accumulate[i] = d.data_ptr(), accumulate
        dwhat = torch.full((3,), float("nan"), device=DEV)
        capi.call("stl_det_fuse_bwd", C.byref(self.f), self.dy.data_ptr(), C.byref(fb), self.ws.data_ptr(), dwhat.data_ptr(), _st())
        torch.cuda.synchronize()
        return dwhat[:self.f.nterms].cpu()


def _check_fuse(kind, S, C, B=2):
    terms, p, dy, hw = _fuse_case(kind, S, C, B)
    dx64, dw64 = _fuse_yardstick(terms, p, dy, hw, torch.float64)
    dx32, dw32 = _fuse_yardstick(terms, p, dy, hw, torch.float32)
    if kind != "up":   # what the planted cases rest on, read off the yardstick
        g = dx64[-1]   # the pooled map's gradient, NHWC
        assert (BR.routed_pool(terms[-1][0])[0, 0, -1, -1] == 0) and g[0, S - 1, S - 1, 0] == 0, \
            "the last pixel of the all-negative channel lies in one window, which the padding wins"
        assert g[1, 1, S % 2, 1] != 0 and g[1, 1, S % 2 + 1, 1] == 0, "the tie's first pixel wins its windows, the second none"
    dev = _FuseBwd(terms, p, dy, hw)
    nan = lambda: [torch.full_like(x, float("nan")) for x in dev.maps]  # noqa: E731
    dx = nan()
    dwhat = dev.run(dx)
    tag = f"fuse_bwd {kind} S={S} C={C}"
    for i in range(len(terms)):
        _hold(f"{tag} dx[{i}]", dx[i], dx64[i], dx32[i], "dx")
        if p[i] <= 0:
            assert not dx[i].any()
    _hold(f"{tag} dwhat", dwhat, dw64, dw32, "dwhat")
    again = nan()
    assert torch.equal(dev.run(again), dwhat) and all(torch.equal(a, b) for a, b in zip(again, dx)), "two runs differ"
    # term 0 frozen: its buffer (handed over nowhere) keeps its canary, the others and dw^ do not change
    canary = [torch.full_like(x, 7.0) for x in dev.maps]
    assert torch.equal(dev.run([None] + canary[1:]), dwhat)
    assert (canary[0] == 7.0).all() and all(torch.equal(a, b) for a, b in zip(canary[1:], dx[1:]))
    # accumulate: base + dx, against the write
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(x.shape, generator=g).to(DEV) for x in dev.maps]
    acc = [b.clone() for b in base]
    dev.run(acc, accumulate=1)
    assert all(torch.equal(a, b + d) for a, b, d in zip(acc, base, dx))


@pytest.mark.parametrize("C_", [8, 160])
@pytest.mark.parametrize("kind,S", FUSE_CASES)
def test_fuse_backward(kind, S, C_):
    _check_fuse(kind, S, C_)


def test_fuse_backward_with_more_than_one_partial_sum():
    """2 x 32 x 32 x 64 outputs: 512 workgroups' partial sums, two per thread of the final sum."""
    _check_fuse("pool3", 64, 64)
    print("fuse_bwd ratios", RATIOS)


def test_fuse_backward_checks_its_arguments():
    terms, p, dy, hw = _fuse_case("pool3", 6, 8)
    dev = _FuseBwd(terms, p, dy, hw)
    dev.f.t[2].H = 7   # 7 x 6 does not pool into 3 x 3
    with pytest.raises(RuntimeError, match="det_fuse_bwd: term 2"):
        dev.run([None, None, None])
    dev.f.t[2].H = 6
    dev.f.wparam = None
    with pytest.raises(RuntimeError, match="det_fuse_bwd"):
        dev.run([None, None, None])


def test_grad_add():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(1000, generator=g).to(DEV), torch.randn(1000, generator=g).to(DEV)
    s = torch.tensor([0.5, 3.0], device=DEV)
    out = torch.empty_like(a)
    capi.call("stl_det_grad_add", a.data_ptr(), b.data_ptr(), None, None, out.data_ptr(), 1000, _st())
    assert torch.equal(out, a + b)
    capi.call("stl_det_grad_add", a.data_ptr(), b.data_ptr(), s.data_ptr(), s[1:].data_ptr(), out.data_ptr(), 1000, _st())
    want = 0.5 * a.double() + 3.0 * b.double()
    bound = 3 * 2.0 ** -24 * (0.5 * a.double().abs() + 3.0 * b.double().abs())   # two products and a sum, each rounded once at most
    assert ((out.double() - want).abs() <= bound).all()
    a0 = a.clone()
    capi.call("stl_det_grad_add", a.data_ptr(), b.data_ptr(), None, None, a.data_ptr(), 1000, _st())   # in place
    assert torch.equal(a, a0 + b)


# ------------------------------------------------------------------------------------------------ the whole method
LEVEL_NODES = ("conv3_up", "conv4_down", "conv5_down", "conv6_down", "conv7_down")   # the nodes whose outputs are a cell's five levels


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).float().cpu()


def _run(cc, ks):
    """One model; per k in ks one detection_loss + backward on the same input, and the plan's maps the yardstick starts from."""
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
    gt, offsets = T.pack_targets(targets, [tuple(c.shape[1:]) for c in chw], 1)
    o["loss_args"] = (torch.from_numpy(m.anchors_np), torch.from_numpy(gt), offsets.tolist())
    return o


def _check_cells(o, cc, k, tag):
    """Every trainable-cell gradient of run k against the yardstick run from the first trainable cell's stored inputs, the pools
    routed by the stored maps."""
    n = len(o["levels"])
    cells = list(range(n - k, n))
    routes = {j: dict(zip(BR.POOLED, o["levels"][j][:4])) for j in cells}
    args = (o["sd"], cc, 1, cells, o["levels"][n - k - 1], routes, *o["loss_args"])
    (c64, r64, g64), (c32, r32, g32) = BR.method_yardstick(*args, torch.float64), BR.method_yardstick(*args, torch.float32)
    run = o["runs"][k]
    _hold(f"{tag} classification", run["loss"]["classification"], c64, c32)
    _hold(f"{tag} regression", run["loss"]["regression"], r64, r32)
    want = {name for name, _ in T.trainable_parameters(o["m"].set_train_bifpn(k))}
    assert set(run["grads"]) == want == set(g64), "a gradient outside trainable_parameters, or one missing"
    for name in sorted(g64):
        if name.startswith("bifpn."):
            assert run["grads"][name].shape == g64[name].shape, name
            _hold(f"{tag} {name}", run["grads"][name], g64[name], g32[name], BR.tensor_class(name))
    print(f"{tag} ratios above the floor", {c: round(v, 2) for c, v in RATIOS.items()})


@pytest.fixture(scope="module")
def d0():
    return _run(0, (0, 1, 2))


@pytest.mark.parametrize("k", [1, 2])
def test_d0_heads_are_bitwise_those_of_k0_and_the_cells_match_the_yardstick(d0, k):
    base, run = d0["runs"][0], d0["runs"][k]
    assert all(torch.equal(run["loss"][n], base["loss"][n]) for n in ("classification", "regression"))
    assert torch.equal(run["reg"], base["reg"]) and torch.equal(run["cls"], base["cls"])
    assert set(base["grads"]) == {n for n, _ in T.head_parameters(d0["m"])}
    for n, g in base["grads"].items():
        assert torch.equal(run["grads"][n], g), n
    _check_cells(d0, 0, k, f"d0 k={k}")
    # k = 1 and k = 2 run the last cell's backward through the same launches
    if k == 2:
        for n, g in d0["runs"][1]["grads"].items():
            assert torch.equal(run["grads"][n], g), n


def test_d3_cell_gradients_match_the_yardstick():
    """C = 160 is no multiple of the 64-wide tile; batch 1."""
    o = _run(3, (1,))
    _check_cells(o, 3, 1, "d3 k=1")


def test_sgd_step_keeps_the_plan_and_refolds_the_tail_exactly(d0):
    m, plan = d0["m"], d0["plan"]
    m.set_train_bifpn(2)
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
    first = m._tail_off[1][0]
    assert torch.equal(m._wbuf, fresh._wbuf) and torch.equal(m._wbuf[:first], before[:first]) and not torch.equal(m._wbuf[first:], before[first:])
    again = m.detection_loss(d0["chw"], d0["targets"])
    sum(again.values()).backward()
    assert all(bool(torch.isfinite(v)) for v in again.values())
    assert not torch.equal(again["classification"], d0["runs"][0]["loss"]["classification"])   # the step moved the network


def test_stale_backward_raises_after_an_inference_forward_too(d0):
    m = d0["m"]
    m.set_train_bifpn(1)
    first = m.detection_loss(d0["chw"], d0["targets"])
    with torch.no_grad():
        m(d0["chw"], postprocess=False)   # overwrites the maps the cells' backward reads
    with pytest.raises(RuntimeError, match="stale forward"):
        sum(first.values()).backward()
    first = m.detection_loss(d0["chw"], d0["targets"])
    m.detection_loss(d0["chw"], d0["targets"])
    with pytest.raises(RuntimeError, match="stale forward"):
        first["classification"].backward()


def test_f16_with_trainable_cells_raises():
    m = E.setup_detector("efficientdet", "d0", compute_dtype="f16").set_train_bifpn(1)
    chw = [torch.zeros(3, 64, 64)]
    with pytest.raises(NotImplementedError, match="fp32"):
        m.detection_loss(chw, [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}])


def test_loss_weights_reach_the_cells(d0):
    """The cells' gradients are linear in the two losses' gradients: 2 * classification + 0.5 * regression."""
    m = d0["m"]
    m.set_train_bifpn(1)
    grads = {}
    for tag, (wc, wr) in (("c", (1.0, 0.0)), ("r", (0.0, 1.0)), ("mix", (2.0, 0.5))):
        for q in m.parameters():
            q.grad = None
        loss = m.detection_loss(d0["chw"], d0["targets"])
        (wc * loss["classification"] + wr * loss["regression"]).backward()
        grads[tag] = {n: q.grad.clone() for n, q in T.trainable_parameters(m) if n.startswith("bifpn.")}
    for n, g in grads["mix"].items():
        want = 2.0 * grads["c"][n].double() + 0.5 * grads["r"][n].double()
        assert (g.double() - want).abs().max() <= 1e-4 * want.abs().max() + 1e-12, n


# ------------------------------------------------------------------------------------------------ DetectorTrainer
def test_detector_trainer_trains_the_last_cell_and_resumes(tmp_path):
    from stlpose_amd.det_data import DetBatchLoader
    from stlpose_amd.detector_trainer import DetectorTrainer
    from stlpose_amd.pose_data import ResidentImages
    from tests import test_det_batch_gpu as DB
    images, db = DB._images(DB.T_SIZES, 21), DB._db(DB.T_SIZES, DB.T_BOXES, DB.T_LABELS)
    store = ResidentImages.from_arrays(images, DEV)

    def trainer(exp_path, **kw):
        exp = DB._exp_data()
        exp["training"]["train_bifpn"] = 1
        model = DB._model(train_header=True)
        train, valid = DetBatchLoader(db, store, exp, 2, True, seed=3), DetBatchLoader(db, store, exp, 2, False)
        return DetectorTrainer(str(exp_path), exp, model, train, valid, db.coco_gt(256), valid_fraction=1.0, **kw)
    t = trainer(tmp_path / "full")
    assert t.model.train_bifpn == 1
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    t.training_loop()
    logs = json.loads((tmp_path / "full" / "detector_logs.json").read_text())
    assert sorted(logs) == ["last_modified", "train_loss", "valid_ap"] and len(logs["train_loss"]) == 2 and t.skipped == 0
    assert all(np.isfinite(logs["train_loss"]))
    after = t.model.state_dict()
    params = {n for n, _ in t.model.named_parameters()}
    for k, v in after.items():
        if k.startswith("bifpn.2.") and k in params:
            assert not torch.equal(v, before[k]), k          # the last cell trains, every parameter of it
        elif not k.startswith(("regressor.", "classifier.")):
            assert torch.equal(v, before[k]), k              # the backbone, the first two cells, every buffer
    saved = tmp_path / "full" / "models" / "detector"
    ck = torch.load(saved / "checkpoint_epoch_final.pth", weights_only=False)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"] and ck["epoch"] == 2
    os.makedirs(tmp_path / "resumed")
    shutil.copy(tmp_path / "full" / "detector_logs.json", tmp_path / "resumed" / "detector_logs.json")
    r = trainer(tmp_path / "resumed", checkpoint=str(saved / "checkpoint_epoch_0.pth"), resume_training=True)
    assert r.cur_epoch == 1
    r.training_loop()
    for k, v in after.items():
        assert torch.equal(v, r.model.state_dict()[k]), k
