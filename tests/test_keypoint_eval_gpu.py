"""GPU: stlpose::pose_rescore_nms / oks_ap_match and stlpose_amd.keypoint_eval against the host functions of evaluate.py, the
reference fixtures G7 / G12 and the numpy yardstick (tests/keypoint_eval_ref.py).

The contract: scores, precision and recall are compared with np.array_equal.  An OKS value may differ from numpy's by the device's
fp64 exp (below 1e-13) and is only ever compared, so every test first asserts that no comparison of the yardstick came closer
than 1e-9 to a tie -- four orders above what exp can move, and far below the spacing random data gives (1e-7 .. 1e-4 here)."""
import json
import os

import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import KeypointGroundTruth, PoseResults, keypoint_ap, keypoint_ap_tables, rescore_and_nms_device
from stlpose_amd.evaluate import COCO_SIGMAS, Evaluator, oks_ap, rescore_and_nms
from tests import keypoint_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIGMAS = [float(s) for s in COCO_SIGMAS]


def _same_results(got, want):
    assert [r["image_id"] for r in got] == [r["image_id"] for r in want]
    assert np.array_equal([r["score"] for r in got], [r["score"] for r in want])
    assert np.array_equal(np.asarray([r["keypoints"] for r in got]), np.asarray([r["keypoints"] for r in want]))
    assert got == want


# ------------------------------------------------------------------------------------------------ reference parity: rescoring + NMS
def _g12(golden_dir, mean_order="numpy"):
    g = np.load(os.path.join(golden_dir, "g12_metrics.npz"))
    _, _, margin = R.rescore_nms_ref(g["sub_kpts"], g["sub_boxes"], g["sub_ids"], mean_order=mean_order)
    assert margin >= 1e-9
    return g, rescore_and_nms_device(g["sub_kpts"], g["sub_boxes"], g["sub_ids"].tolist(), device=DEV, mean_order=mean_order)


def test_g12_generate_submission_kept_persons(golden_dir):
    """fixture G12: the reference's generate_submission_hrnet on 20 persons in 4 images (smallest |OKS - 0.9|: 0.085), in the
    default summation order (the host function's): the kept counts, the image order and the keypoints, exactly; the scores as
    test_evaluate_cpu.py pins the host function (rtol 1e-12: numpy's mean() is one ulp from the reference's loop in 3 of the 16)."""
    g, res = _g12(golden_dir)
    assert np.diff(res.offsets).tolist() == g["sub_kept_n"].tolist()
    assert np.repeat(res.image_ids, np.diff(res.offsets)).tolist() == g["sub_kept_img"].tolist()
    assert np.array_equal(res.keypoints.cpu().numpy(), g["sub_kept_kpts"])
    np.testing.assert_allclose(res.scores.cpu().numpy(), g["sub_kept_scores"], rtol=1e-12)


def test_g12_generate_submission_scores_exactly(golden_dir):
    """fixture G12 with np.array_equal throughout: kept counts, image order, keypoints and scores.  The reference sums the confident
    joints one after the other (lib/metrics.py:242-250); mean_order="reference" does the same on the device.  (The default order
    is numpy's, to equal evaluate.rescore_and_nms bit for bit; on G12 that is one ulp away in 3 of the 16 scores.)"""
    g, res = _g12(golden_dir, "reference")
    assert np.diff(res.offsets).tolist() == g["sub_kept_n"].tolist()
    assert np.repeat(res.image_ids, np.diff(res.offsets)).tolist() == g["sub_kept_img"].tolist()
    assert np.array_equal(res.keypoints.cpu().numpy(), g["sub_kept_kpts"])
    got, want = res.scores.cpu().numpy(), g["sub_kept_scores"]
    print("G12 scores: %d of %d differ, max |diff| %.3g" % ((got != want).sum(), len(want), np.abs(got - want).max()))
    assert np.array_equal(got, want)
    host = rescore_and_nms(g["sub_kpts"], g["sub_boxes"], g["sub_ids"].tolist())
    assert not np.array_equal([r["score"] for r in host], want)           # the two orders do differ here


@pytest.mark.parametrize("thr,key", [(0.9, "keep_09"), (0.5, "keep_05")])
def test_g7_oks_nms_through_the_op(golden_dir, thr, key):
    """fixture G7: the reference's own lib/nms.py outputs for six persons.  Confidence 1 everywhere makes the op's score the given one."""
    g = np.load(os.path.join(golden_dir, "g7_decode.npz"))
    preds = g["nms_kpts"].copy()
    preds[:, :, 2] = 1.0
    boxes = np.zeros((6, 6))
    boxes[:, 4], boxes[:, 5] = g["nms_areas"], g["nms_scores"]
    score, keep, count = torch.ops.stlpose.pose_rescore_nms(torch.from_numpy(preds).to(DEV), torch.from_numpy(boxes).to(DEV),
                                                            torch.tensor([0, 6]), 0.2, thr, SIGMAS)
    assert np.array_equal(score.cpu().numpy(), g["nms_scores"])
    n = int(count[0])
    assert keep[:n].cpu().tolist() == g[key].tolist() and (keep[n:] == -1).all()


# ------------------------------------------------------------------------------------------------ NMS against the host function
@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["float32", "float64"])
def nms_case(request):
    preds, boxes, ids = R.nms_set(dtype=request.param)
    kept, scores, margin = R.rescore_nms_ref(preds, boxes, ids)
    return preds, boxes, ids, scores, margin, rescore_and_nms(preds, boxes, ids.tolist())


def test_nms_equals_the_host_function(nms_case):
    preds, boxes, ids, scores, margin, want = nms_case
    sizes = []
    for im in dict.fromkeys(ids.tolist()):
        sc = scores[ids == im]
        sizes.append(len(sc))
        if len(sc) > 16:
            assert len(np.unique(sc)) == len(sc)                      # ties only where argsort()[::-1] has a defined order
    assert sorted(sizes) == list(R.NMS_SIZES)
    small = [im for im in np.unique(ids) if (ids == im).sum() <= 16]
    assert any((scores[ids == im] == 0).sum() >= 3 for im in small)   # several zero scores tied in one image
    assert margin >= 1e-9
    res = rescore_and_nms_device(preds, boxes, ids.tolist(), device=DEV)
    assert 1 < len(want) < len(preds)                                 # something is suppressed, something kept
    _same_results(res.to_list(), want)
    # tensors in, the persons of each image adjacent already
    order = np.argsort(ids, kind="stable")
    res2 = rescore_and_nms_device(torch.from_numpy(preds[order]).to(DEV), torch.from_numpy(boxes[order]), ids[order], device=DEV)
    by_img = {}
    for r in want:
        by_img.setdefault(r["image_id"], []).append(r)
    _same_results(res2.to_list(), [r for im in sorted(by_img) for r in by_img[im]])


def test_reference_summation_order(nms_case):
    """mean_order="reference" on the ragged set: the scores of the reference's running sum, bit for bit, in both dtypes, and the
    suppression that follows from them."""
    preds, boxes, ids, numpy_scores, *_ = nms_case
    kept, scores, margin = R.rescore_nms_ref(preds, boxes, ids, mean_order="reference")
    assert margin >= 1e-9 and not np.array_equal(scores, numpy_scores)
    for im in np.unique(ids):
        sc = scores[ids == im]
        assert len(sc) <= 16 or len(np.unique(sc)) == len(sc)
    res = rescore_and_nms_device(preds, boxes, ids.tolist(), device=DEV, mean_order="reference")
    rows = [r for _, k in kept for r in k]
    assert np.repeat(res.image_ids, np.diff(res.offsets)).tolist() == [im for im, k in kept for _ in k]
    assert np.array_equal(res.scores.cpu().numpy(), scores[rows])
    assert np.array_equal(res.keypoints.cpu().numpy(), preds[rows].astype(np.float64))


def test_nms_other_thresholds(nms_case):
    preds, boxes, ids, *_ = nms_case
    sel = np.isin(ids, [100, 101, 102, 103, 104, 105])
    p, b, i = preds[sel], boxes[sel], ids[sel]
    _, _, margin = R.rescore_nms_ref(p, b, i, in_vis_thr=0.5, oks_thr=0.6)
    assert margin >= 1e-9
    _same_results(rescore_and_nms_device(p, b, i.tolist(), in_vis_thr=0.5, oks_thr=0.6, device=DEV).to_list(),
                  rescore_and_nms(p, b, i.tolist(), in_vis_thr=0.5, oks_thr=0.6))


# ------------------------------------------------------------------------------------------------ AP against the yardstick
@pytest.fixture(scope="module")
def ap_case():
    gts, dts = R.ap_set()
    return gts, dts, KeypointGroundTruth(gts, device=DEV)


@pytest.mark.parametrize("max_dets,subset", [(20, False), (5, False), (20, True)])
def test_ap_equals_the_yardstick(ap_case, max_dets, subset):
    gts, dts, table = ap_case
    ids = list(range(2, 70, 2)) if subset else None                   # 66 and 68 name no image at all
    want = R.keypoint_ap_ref(gts, dts, img_ids=ids, max_dets=max_dets)
    assert want["margin"] >= 1e-9
    assert ((want["stats"] > 0) & (want["stats"] < 1)).all()
    got = keypoint_ap_tables(gts, dts, img_ids=ids, max_dets=max_dets, device=DEV)
    assert got.precision.shape == (10, 101, 3) and got.recall.shape == (10, 3)
    assert got.precision.flags["C_CONTIGUOUS"] and got.recall.flags["C_CONTIGUOUS"]
    assert np.array_equal(got.recall, want["recall"])
    assert np.array_equal(got.precision, want["precision"])
    assert np.array_equal(got.stats, oks_ap(gts, dts, img_ids=ids, max_dets=max_dets))
    assert np.array_equal(keypoint_ap(table, dts, img_ids=ids, max_dets=max_dets), got.stats)     # the table built once


def test_ap_from_pose_results(ap_case):
    """A PoseResults (no "area": the keypoints' bounding box) scores like its list."""
    gts, dts, table = ap_case
    dts = sorted((dict(d) for d in dts), key=lambda d: -d["image_id"])               # images adjacent, descending ids
    for d in dts:
        d.pop("area", None)
    want = R.keypoint_ap_ref(gts, dts)
    assert want["margin"] >= 1e-9
    res = PoseResults.from_list(dts, device=DEV)
    got = keypoint_ap_tables(table, res)
    assert np.array_equal(got.precision, want["precision"]) and np.array_equal(got.recall, want["recall"])
    assert np.array_equal(got.stats, oks_ap(gts, dts))


@pytest.mark.parametrize("name", ["perfect", "half", "straddle", "ignored"])
def test_ap_hand_cases(name):
    gts, dts = R.hand_cases()[name]
    want = R.keypoint_ap_ref(gts, dts)
    assert want["margin"] >= 1e-9
    s = keypoint_ap(gts, dts, device=DEV)
    assert np.array_equal(s, oks_ap(gts, dts))
    if name == "perfect":
        assert np.allclose(s, 1.0)
    elif name == "half":
        assert np.isclose(s[0], 51 / 101) and np.isclose(s[5], 0.5)
    elif name == "straddle":
        assert np.isclose(s[1], 1.0) and np.isclose(s[2], 0.0) and 0.0 < s[0] < 1.0
    else:
        assert np.isclose(s[0], 1.0) and np.isclose(s[5], 1.0) and s[4] == -1.0


def test_ap_without_results_or_ground_truth():
    gts, dts = R.hand_cases()["perfect"]
    assert np.array_equal(keypoint_ap(gts, [], device=DEV), oks_ap(gts, []))
    assert np.array_equal(keypoint_ap([], dts, device=DEV), oks_ap([], dts))
    assert np.array_equal(keypoint_ap([], [], device=DEV), oks_ap([], []))


# ------------------------------------------------------------------------------------------------ the op's slots
def test_match_slots():
    """Two images; the first has a far detection listed before one whose OKS straddles the thresholds."""
    g1, g2 = R.person(100, 100, 1, 1), R.person(150, 150, 2, 2, area=120.0 * 120.0)
    dts = [R.det(g1, 0.3, shift=500.0), R.det(g1, 0.9, shift=R.straddle_shift(g1)), R.det(g2, 0.5)]
    v = float(R.oks_tile([dts[1]], [g1], COCO_SIGMAS)[0, 0])
    assert 0.55 < v < 0.7 and np.abs(v - R.OKS_THRS).min() >= 1e-9
    table = KeypointGroundTruth([g1, g2], device=DEV)
    kp = torch.tensor([d["keypoints"] for d in dts], dtype=torch.float64, device=DEV).reshape(-1, 17, 3)
    sc = torch.tensor([d["score"] for d in dts], dtype=torch.float64, device=DEV)
    out = torch.ops.stlpose.oks_ap_match(kp, sc, None, torch.tensor([0, 2, 3]), *table.select(np.array([1, 2])),
                                         [float(t) for t in R.OKS_THRS], [float(x) for r in R.AREA_RANGES for x in r], SIGMAS)
    score, cat, rank, matched, ignored, npig = (t.cpu().numpy() for t in out)
    assert score.tolist() == [0.9, 0.3, 0.5] and cat.tolist() == [0, 0, 0] and rank.tolist() == [0, 1, 0]
    assert npig.tolist() == [[[1, 1, 0]], [[1, 0, 1]]]
    bit = lambda w, t, a: int(w >> (t * 3 + a)) & 1
    for t, thr in enumerate(R.OKS_THRS):
        for a in range(3):
            # the straddling one: matched below its OKS; the ground truth is outside "large", and so is the detection's own box
            assert bit(matched[0], t, a) == int(v >= thr)
            assert bit(ignored[0], t, a) == int(a == 2)
            # the far one matches nothing
            assert bit(matched[1], t, a) == 0 and bit(ignored[1], t, a) == int(a == 2)
            # the exact one of image 2 (area 120^2: outside "medium") always matches
            assert bit(matched[2], t, a) == 1 and bit(ignored[2], t, a) == int(a == 1)
    assert (matched >> 30 == 0).all() and (ignored >> 30 == 0).all()


def test_two_runs_are_bitwise_equal(ap_case):
    gts, dts, table = ap_case
    a, b = keypoint_ap_tables(table, dts), keypoint_ap_tables(table, dts)
    assert np.array_equal(a.precision, b.precision) and np.array_equal(a.recall, b.recall)
    preds, boxes, ids = R.nms_set(dtype=np.float32)
    x, y = (rescore_and_nms_device(preds, boxes, ids, device=DEV) for _ in range(2))
    assert torch.equal(x.scores, y.scores) and torch.equal(x.keypoints, y.keypoints) and np.array_equal(x.offsets, y.offsets)


def test_caps_name_the_image():
    gts = [R.person(100, 100, 9, i) for i in range(129)] + [R.person(100, 100, 4, 500)]
    with pytest.raises(ValueError, match="image_id 9: .*position 1 has 129 ground truths.*STL_BOX_AP_GT_MAX"):
        keypoint_ap(gts, [R.det(gts[0], 0.5)], device=DEV)
    preds, boxes = np.zeros((1027, 17, 3), np.float32), np.zeros((1027, 6))
    with pytest.raises(ValueError, match="image_id 31: 1025 persons.*STL_POSE_NMS_MAX"):
        rescore_and_nms_device(preds, boxes, [30] + [31] * 1025 + [32], device=DEV)


# ------------------------------------------------------------------------------------------------ the evaluation driver
def _loader(nbatch=6, per=5):
    rng = np.random.Generator(np.random.PCG64(5))
    out = []
    for b in range(nbatch):
        n = per if b != nbatch - 1 else per - 2
        meta = dict(center=rng.random((n, 2)) * 400 + 100, scale=0.5 + rng.random((n, 2)), score=rng.random(n),
                    image_id=np.array([100 + ((b * per + i) * 7 % 11) for i in range(n)]))      # an image's persons in several batches
        out.append((np.full((n, 1), b, np.float32), None, None, meta))
    return out


class _Fake(Evaluator):
    def __init__(self, scoring):
        self.model, self.pg, self.shard_loader, self.rank, self.world = None, None, True, 0, 1
        self.scoring, self.device = scoring, torch.device(DEV)

    def _batch_outputs(self, imgs, target, target_weight, centers, scales):
        b = int(imgs[0, 0])
        rng = np.random.Generator(np.random.PCG64(1000 + b))
        n = len(centers)
        kp = rng.random((n, 17, 2)) * 150 + centers[:, None, :]
        if n > 1:
            kp[1] = kp[0] + 0.5             # a near-duplicate for the NMS
        return 0.1 * (b + 1), 0.05 * b, kp, rng.random((n, 17, 1))


def test_evaluator_device_scoring_equals_host_scoring(tmp_path):
    loader = _loader()
    host = _Fake("host").evaluate_model(loader, preds_file=str(tmp_path / "host.json"))
    # ground truth near some of the kept persons, so that the ten numbers are not trivial
    rng = np.random.Generator(np.random.PCG64(9))
    gts = []
    for i, r in enumerate(host["results"][::2]):
        k = np.asarray(r["keypoints"]).reshape(17, 3).copy()
        k[:, :2] += rng.normal(0, rng.choice([1.0, 4.0, 10.0]), (17, 2))
        k[:, 2] = 2
        gts.append(dict(id=i, image_id=r["image_id"], category_id=1, keypoints=k.reshape(-1).tolist(), num_keypoints=17,
                        area=float(np.ptp(k[:, 0]) * np.ptp(k[:, 1]) * 0.7), bbox=[float(k[:, 0].min()), float(k[:, 1].min()),
                                                                                float(np.ptp(k[:, 0])), float(np.ptp(k[:, 1]))], iscrowd=0))
    assert R.keypoint_ap_ref(gts, host["results"])["margin"] >= 1e-9
    host = _Fake("host").evaluate_model(loader, gt_annotations=gts, preds_file=str(tmp_path / "host.json"))
    dev = _Fake("device").evaluate_model(loader, gt_annotations=gts, preds_file=str(tmp_path / "device.json"))
    assert len(host["results"]) > 10 and 0 < host["stats"][0] < 1
    _same_results(dev["results"], host["results"])
    assert np.array_equal(dev["stats"], host["stats"])
    assert dev["loss"] == host["loss"] and dev["accuracy"] == host["accuracy"]
    assert (tmp_path / "device.json").read_bytes() == (tmp_path / "host.json").read_bytes()
    assert json.loads((tmp_path / "device.json").read_text()) == host["results"]
    assert _Fake("device").evaluate_model(loader)["stats"] is None
