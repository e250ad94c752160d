"""GPU: stlpose::eval_tail / eval_affine, eval_tail.EvalTables and Evaluator(tail="device") against the numpy yardstick
(tests/eval_tail_ref.py) and against the host tail.

The contract: arg-max coordinates, refined coordinates, maxval and the decoded keypoints are compared with np.array_equal.  A
batch's loss is the float32 of an fp64 sum of non-negative terms over n <= 2^22 elements: any summation order errs below
n * 2^-53 <= 2^-31 relative, and the one cast to float32 can then move the result by at most one ulp, so it must be np.float32 of
the yardstick's float64 value or a neighbouring float32.  The mean of per-batch losses that differ by at most one ulp each
differs by at most 2^-23 relative."""
import json

import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd.eval_tail import EvalTables
from stlpose_amd.evaluate import Evaluator
from tests import eval_tail_ref as R
from tests import keypoint_eval_ref as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run_op(a, bf, t, tw, row0=0, rows=None):
    b, j, h, w = a.shape
    rows = row0 + b if rows is None else rows
    tabs = [torch.full((rows, *tail), -7.0, dtype=torch.float32, device=DEV) for tail in ((j, 2), (j, 2), (j, 2), (j,))]
    partial = torch.zeros(b * j, dtype=torch.float64, device=DEV)
    losses = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    torch.ops.stlpose.eval_tail(_dev(a), _dev(bf), _dev(R.perm(j)), _dev(t), _dev(tw), *tabs, partial, losses, row0, 1)
    return tabs, partial, losses


def _check_loss(got, want64):
    if np.isnan(want64):
        assert np.isnan(got)
    else:
        assert float(got) in R.float32_neighbours(want64), (float(got), want64)


@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_equals_the_yardstick(shape, flip):
    a, bf, t, tw = R.case(shape, seed=11)
    if not flip:
        bf = None
    y = R.tail(a, bf, t, tw)
    b, j, h, w = shape
    (pred_xy, tgt_xy, coords, maxval), partial, losses = _run_op(a, bf, t, tw, row0=2, rows=b + 3)
    for name, tab in (("pred_xy", pred_xy), ("tgt_xy", tgt_xy), ("coords", coords), ("maxval", maxval)):
        got = tab.cpu().numpy()
        assert np.array_equal(got[2:2 + b], y[name]), name
        assert (got[:2] == -7).all() and (got[2 + b:] == -7).all(), name   # rows of other batches are not touched
    losses = losses.cpu().numpy()
    print(f"loss {losses[1]!r} yardstick {y['loss']!r}")
    _check_loss(losses[1], y["loss"])
    assert losses[0] == -7 and losses[2] == -7
    assert np.allclose(partial.cpu().numpy().reshape(b, j), y["partial"], rtol=2.0 ** -31, atol=0)
    # eval_affine over the rows against final_preds on the materialised flip_merge output
    rng = np.random.Generator(np.random.PCG64(2))
    c, s = (rng.random((b, 2)) * 300 + 100).astype(np.float32), (rng.random((b, 2)) + 0.5).astype(np.float32)
    preds = torch.ops.stlpose.eval_affine(coords[2:].contiguous(), maxval[2:].contiguous(), _dev(c), _dev(s), h, w).cpu().numpy()
    hm = _dev(a) if bf is None else torch.ops.stlpose.flip_merge(_dev(a), _dev(bf), _dev(R.perm(j)))
    assert np.array_equal(hm.cpu().numpy(), y["merged"])
    want, mx = torch.ops.stlpose.final_preds(hm, _dev(c), _dev(s))
    assert preds.shape == (b, j, 3)
    assert np.array_equal(preds[..., :2], want.cpu().numpy()) and np.array_equal(preds[..., 2:], mx.cpu().numpy())
    assert np.array_equal(preds, R.affine(y["coords"], y["maxval"], c, s, h, w))


def test_nan_map():
    a, bf, t, tw = R.case((2, 17, 33, 31), seed=12, nan=True)
    y = R.tail(a, bf, t, tw)
    (pred_xy, tgt_xy, coords, maxval), partial, losses = _run_op(a, bf, t, tw)
    assert np.isnan(y["maxval"][1, 16]) and np.array_equal(y["coords"][1, 16], [0, 0])
    for name, tab in (("pred_xy", pred_xy), ("tgt_xy", tgt_xy), ("coords", coords), ("maxval", maxval)):
        assert np.array_equal(tab.cpu().numpy(), y[name], equal_nan=True), name
    _check_loss(losses.cpu().numpy()[1], y["loss"])


def test_two_runs_are_bitwise_equal():
    a, bf, t, tw = R.case((2, 17, 96, 72), seed=13)
    one, two = _run_op(a, bf, t, tw), _run_op(a, bf, t, tw)
    for x, y in zip(one[0] + [one[1], one[2]], two[0] + [two[1], two[2]]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_op_refuses_tables_that_are_too_small():
    a, bf, t, tw = R.case((2, 17, 5, 7), seed=1)
    with pytest.raises(ValueError, match="pred_xy"):
        _run_op(a, bf, t, tw, row0=3, rows=4)


# ------------------------------------------------------------------------------------------------ the tables
def test_table_growth():
    """4200 persons in 300 batches of 14: past the 4096 rows and the 256 loss slots the tables start with."""
    shape = (4200, 17, 5, 7)
    a, bf, t, tw = R.case(shape, seed=21)
    y = R.tail(a, bf, t, tw)
    rng = np.random.Generator(np.random.PCG64(4))
    c, s = rng.random((4200, 2)) * 300 + 100, rng.random((4200, 2)) + 0.5
    tables = EvalTables(DEV)
    assert tables._tables[0].shape[0] == 4096 == EvalTables.ROWS
    da, dbf, dt, dtw = _dev(a), _dev(bf), _dev(t), _dev(tw)
    for r in range(0, 4200, 14):
        tables.add(da[r:r + 14], dbf[r:r + 14], dt[r:r + 14], dtw[r:r + 14])
    assert tables._tables[0].shape[0] == 8192 and tables._losses.numel() == 512
    preds, losses, pcks = tables.finish(c, s)
    assert np.array_equal(preds, R.affine(y["coords"], y["maxval"], c, s, 5, 7))
    assert np.array_equal(tables.preds.cpu().numpy(), preds)
    assert len(losses) == len(pcks) == 300
    from stlpose_amd.pose_parsing import pck_from_coords
    for k in (0, 1, 150, 292, 293, 299):   # 4096 = 292 * 14 + 8: the batch that crosses the first table's end, and its neighbours
        r = slice(14 * k, 14 * k + 14)
        _check_loss(np.float32(losses[k]), y["partial"][r].sum() * 0.5 / (14 * 17 * 35))
        assert pcks[k] == pck_from_coords(y["pred_xy"][r], y["tgt_xy"][r], 5, 7)[1]


# ------------------------------------------------------------------------------------------------ the evaluation driver
class _Stub(torch.nn.Module):
    """Returns prepared heat maps: an image carries 1 + its person's row in pixel (0, 0) and the negative of it in the last pixel
    of that row, so the mirrored image asks for the maps of the mirrored pass.  A device gather, no sync."""

    def __init__(self, maps, maps_flipped):
        super().__init__()
        self.register_buffer("maps", torch.from_numpy(maps))
        self.register_buffer("maps_flipped", torch.from_numpy(maps_flipped))

    def forward(self, img):
        v = img[:, 0, 0, 0]
        rows = v.abs().long() - 1
        return torch.where((v < 0)[:, None, None, None], self.maps_flipped[rows], self.maps[rows])


def _epoch(nan=False, sizes=(4, 4, 3), h=16, w=12, seed=31):
    """Three batches of 4, 4 and 3 persons, three persons per image (so an image's persons lie in two batches), blobs on a noisy
    background; person 1 repeats person 0 half a pixel away (a near-duplicate for the NMS)."""
    n = sum(sizes)
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]

    def blobs(cy, cx):
        g = np.exp(-((yy - cy[..., None, None]) ** 2 + (xx - cx[..., None, None]) ** 2) / 4.0)
        return (g * (0.3 + 0.7 * rng.random((n, 17, 1, 1))) + 0.05 * rng.random((n, 17, h, w))).astype(np.float32)
    cy, cx = rng.random((n, 17)) * (h - 1), rng.random((n, 17)) * (w - 1)
    maps = blobs(cy, cx)
    mirrored = blobs(cy + rng.normal(0, 0.4, (n, 17)), (w - 1 - cx) + rng.normal(0, 0.4, (n, 17)))[:, R.perm(17)]
    target = blobs(cy + rng.normal(0, 1.0, (n, 17)), cx + rng.normal(0, 1.0, (n, 17)))
    target[2, 3] = 0                        # a joint without annotation
    maps[1], mirrored[1] = maps[0], mirrored[0]
    if nan:
        maps[5, 2, 3, 4] = np.nan
    tw = rng.choice(np.asarray([0.0, 1.0, 1.0], np.float32), (n, 17, 1))
    centers, scales = rng.random((n, 2)) * 400 + 100, 0.5 + rng.random((n, 2))
    centers[1], scales[1] = centers[0] + 0.5, scales[0]
    score, ids = rng.random(n), 100 + np.arange(n) // 3
    img = np.zeros((n, 1, 1, 2), np.float32)
    img[:, 0, 0, 0], img[:, 0, 0, 1] = 1 + np.arange(n), -(1 + np.arange(n))
    batches, r = [], 0
    for b in sizes:
        q = slice(r, r + b)
        batches.append((torch.from_numpy(img[q]), torch.from_numpy(target[q]), torch.from_numpy(tw[q]),
                        dict(center=centers[q], scale=scales[q], score=score[q], image_id=ids[q])))
        r += b
    model = _Stub(maps, mirrored).to(DEV)
    y = R.tail(maps, mirrored, target, tw)
    preds = R.affine(y["coords"], y["maxval"], centers, scales, h, w)
    boxes = np.zeros((n, 6))
    boxes[:, 0:2], boxes[:, 2:4], boxes[:, 4], boxes[:, 5] = centers, scales, np.prod(scales * 200, 1), score
    return model, batches, preds, boxes, ids


def _ground_truth(results):
    rng = np.random.Generator(np.random.PCG64(9))
    gts = []
    for i, r in enumerate(results[::2]):
        k = np.asarray(r["keypoints"]).reshape(17, 3).copy()
        k[:, :2] += rng.normal(0, rng.choice([1.0, 4.0, 10.0]), (17, 2))
        k[:, 2] = 2
        gts.append(dict(id=i, image_id=r["image_id"], category_id=1, keypoints=k.reshape(-1).tolist(), num_keypoints=17,
                        area=float(np.ptp(k[:, 0]) * np.ptp(k[:, 1]) * 0.7),
                        bbox=[float(k[:, 0].min()), float(k[:, 1].min()), float(np.ptp(k[:, 0])), float(np.ptp(k[:, 1]))], iscrowd=0))
    return gts


@pytest.mark.parametrize("scoring", ["host", "device"])
def test_evaluator_device_tail_equals_host_tail(scoring, tmp_path):
    model, batches, preds, boxes, ids = _epoch()
    if scoring == "device":
        assert K.rescore_nms_ref(preds, boxes, ids)[2] >= 1e-9
    first = Evaluator(model, device=DEV, scoring="host").evaluate_model(batches)
    gts = _ground_truth(first["results"])
    if scoring == "device":
        assert K.keypoint_ap_ref(gts, first["results"])["margin"] >= 1e-9
    host = Evaluator(model, device=DEV, scoring=scoring, tail="host").evaluate_model(batches, gt_annotations=gts,
                                                                                       preds_file=str(tmp_path / "host.json"))
    dev = Evaluator(model, device=DEV, scoring=scoring, tail="device").evaluate_model(batches, gt_annotations=gts,
                                                                                       preds_file=str(tmp_path / "device.json"))
    assert set(dev) == set(host) == {"loss", "accuracy", "results", "stats"}
    assert len(host["results"]) >= 8 and 0 < host["accuracy"] < 1
    assert dev["results"] == host["results"]
    assert dev["accuracy"] == host["accuracy"]
    assert np.array_equal(dev["stats"], host["stats"])
    print(f"loss device tail {dev['loss']!r} host tail {host['loss']!r}")
    assert abs(dev["loss"] - host["loss"]) <= 2.0 ** -23 * host["loss"]
    assert (tmp_path / "device.json").read_bytes() == (tmp_path / "host.json").read_bytes()
    assert json.loads((tmp_path / "device.json").read_text()) == host["results"]


def test_evaluator_without_flip_and_without_batches():
    model, batches, *_ = _epoch()
    host = Evaluator(model, device=DEV, flip=False).evaluate_model(batches)
    dev = Evaluator(model, device=DEV, flip=False, tail="device").evaluate_model(batches)
    assert dev["results"] == host["results"] and dev["accuracy"] == host["accuracy"] and dev["stats"] is None
    assert abs(dev["loss"] - host["loss"]) <= 2.0 ** -23 * host["loss"]
    empty = Evaluator(model, device=DEV, tail="device").evaluate_model([])
    assert empty["results"] == [] and np.isnan(empty["loss"])


def test_evaluator_on_the_network():
    """The real model in the loop (tiny HRNet, fp32, 64 x 64 crops -> 16 x 16 maps): the device tail calls it directly."""
    from stlpose_amd import PoseHighResolutionNet
    torch.manual_seed(0)
    model = PoseHighResolutionNet("tiny", "fp32").to(DEV).eval()
    rng = np.random.Generator(np.random.PCG64(41))
    g = torch.Generator().manual_seed(3)
    batches = []
    for bi, n in enumerate((3, 2)):
        batches.append((torch.randn(n, 3, 64, 64, generator=g), torch.rand(n, 17, 16, 16, generator=g), torch.ones(n, 17, 1),
                        dict(center=rng.random((n, 2)) * 300 + 100, scale=0.5 + rng.random((n, 2)), score=rng.random(n),
                             image_id=np.full(n, 7 + bi))))
    host = Evaluator(model, device=DEV).evaluate_model(batches)
    dev = Evaluator(model, device=DEV, tail="device").evaluate_model(batches)
    assert len(host["results"]) >= 2 and dev["results"] == host["results"] and dev["accuracy"] == host["accuracy"]
    assert abs(dev["loss"] - host["loss"]) <= 2.0 ** -23 * host["loss"]


def test_non_finite_heat_maps_raise():
    model, batches, *_ = _epoch(nan=True)
    with pytest.raises(FloatingPointError, match="non-finite heat maps"):
        Evaluator(model, device=DEV, tail="device").evaluate_model(batches)


# ------------------------------------------------------------------------------------------------ no sync in the loop
class _Watch:
    """While the loader is between its first yield and its end: sync debug mode 'error' (where this build of torch honours it) and a
    count of the calls that copy to the host or wait for the device."""

    def __init__(self, monkeypatch, batches, use_debug_mode):
        self.active, self.calls, self.batches, self.use_debug_mode = False, [], batches, use_debug_mode
        for name in ("item", "cpu", "tolist", "numpy"):
            monkeypatch.setattr(torch.Tensor, name, self._counted(name, getattr(torch.Tensor, name)))
        monkeypatch.setattr(torch.cuda, "synchronize", self._counted("synchronize", torch.cuda.synchronize))

    def _counted(self, name, fn):
        def wrapper(*args, **kwargs):
            if self.active:
                self.calls.append(name)
            return fn(*args, **kwargs)
        return wrapper

    def _set(self, on):
        self.active = on
        if self.use_debug_mode:
            torch.cuda.set_sync_debug_mode("error" if on else "default")

    def loader(self):
        try:
            for i, batch in enumerate(self.batches):
                if i == 0:
                    self._set(True)
                yield batch
        finally:
            self._set(False)


def _item_raises_under_sync_debug_mode():
    x = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_no_sync_between_the_first_and_the_last_batch(monkeypatch):
    model, batches, *_ = _epoch()
    want = Evaluator(model, device=DEV, tail="device").evaluate_model(batches)   # also warms up: lazy initialisation may sync
    Evaluator(model, device=DEV, tail="host").evaluate_model(batches)
    honoured = _item_raises_under_sync_debug_mode()
    print("sync debug mode 'error' raises on .item():", honoured)
    watch = _Watch(monkeypatch, batches, honoured)
    got = Evaluator(model, device=DEV, tail="device").evaluate_model(watch.loader())
    assert not watch.active and watch.calls == []
    assert got["results"] == want["results"] and got["loss"] == want["loss"] and got["accuracy"] == want["accuracy"]
    # the same harness trips on the host tail: the check can fail
    watch = _Watch(monkeypatch, batches, honoured)
    try:
        Evaluator(model, device=DEV, tail="host").evaluate_model(watch.loader())
        tripped = False
    except RuntimeError as e:
        tripped = "synchroniz" in str(e)
        assert tripped, e
    finally:
        watch._set(False)
    assert honoured == tripped
    assert tripped or len(watch.calls) > 0
    if not honoured:
        assert {"item", "cpu"} <= set(watch.calls)
