"""CPU: the yardstick of the device pose scoring (tests/keypoint_eval_ref.py) against the host functions of evaluate.py, the
argument checks of the two ops and of the public functions (everything is refused before a launch), and PoseResults."""
import numpy as np
import pytest
import torch

from stlpose_amd import capi
from stlpose_amd.evaluate import COCO_SIGMAS, oks_ap, rescore_and_nms

from tests import keypoint_eval_ref as R


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", ["perfect", "half", "straddle", "ignored"])
def test_yardstick_equals_oks_ap_on_the_hand_cases(name):
    gts, dts = R.hand_cases()[name]
    ref = R.keypoint_ap_ref(gts, dts)
    assert np.array_equal(ref["stats"], oks_ap(gts, dts))
    assert ref["precision"].shape == (10, 101, 3) and ref["recall"].shape == (10, 3)
    if name == "ignored":
        assert ref["stats"][4] == -1.0 and (ref["precision"][:, :, 2] == -1).all()


@pytest.mark.parametrize("max_dets,subset", [(20, False), (5, False), (20, True)])
def test_yardstick_equals_oks_ap_on_the_random_set(max_dets, subset):
    gts, dts = R.ap_set()
    ids = list(range(2, 70, 2)) if subset else None
    ref = R.keypoint_ap_ref(gts, dts, img_ids=ids, max_dets=max_dets)
    assert np.array_equal(ref["stats"], oks_ap(gts, dts, img_ids=ids, max_dets=max_dets))
    assert ref["margin"] >= 1e-9
    assert ((ref["stats"] > 0) & (ref["stats"] < 1)).all()           # not degenerate


def test_random_set_has_the_cases_it_promises():
    gts, dts = R.ap_set()
    per_gt = np.bincount([g["image_id"] for g in gts], minlength=65)
    per_dt = np.bincount([d["image_id"] for d in dts], minlength=65)
    assert per_gt.max() == 128 and 65 in per_gt and per_dt.max() >= 30
    assert ((per_gt[1:] == 0) & (per_dt[1:] > 0)).any() and ((per_gt[1:] > 0) & (per_dt[1:] == 0)).any()
    assert any(g["iscrowd"] for g in gts) and any(g["num_keypoints"] == 0 for g in gts)
    assert any(0 < g["num_keypoints"] < 17 for g in gts)
    assert any(g["area"] == 32.0 ** 2 for g in gts) and any(g["area"] == 96.0 ** 2 for g in gts)
    assert len({d["image_id"] for d in dts if d["score"] == 0.0}) > 1
    assert any("area" in d for d in dts) and any("area" not in d for d in dts)


def test_nms_yardstick_equals_rescore_and_nms():
    preds, boxes, ids = R.nms_set(dtype=np.float32)
    kept, scores, margin = R.rescore_nms_ref(preds, boxes, ids)
    res = rescore_and_nms(preds, boxes, ids.tolist())
    rows = [r for _, k in kept for r in k]
    assert margin >= 1e-9
    assert [r["image_id"] for r in res] == [im for im, k in kept for _ in k]
    assert np.array_equal([r["score"] for r in res], scores[rows])
    assert np.array_equal(np.array([r["keypoints"] for r in res]).reshape(-1, 17, 3), preds[rows].astype(np.float64))


# ------------------------------------------------------------------------------------------------ the wrappers refuse before a launch
def _nms_args(n=3):
    return [torch.zeros(n, 17, 3), torch.zeros(n, 6, dtype=torch.float64), torch.tensor([0, n]), 0.2, 0.9, [float(s) for s in COCO_SIGMAS]]


def test_rescore_nms_wrapper_refuses_before_launch():
    from stlpose_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops._pose_rescore_nms(*_nms_args())
    for i, bad, word in ((0, torch.zeros(3, 17, 3, dtype=torch.float16), "float32 or float64"), (0, torch.zeros(3, 16, 3), "17, 3"),
                         (1, torch.zeros(3, 6), "float64"), (1, torch.zeros(3, 5, dtype=torch.float64), "boxes"),
                         (2, torch.tensor([0, 2]), "offsets"), (2, torch.tensor([0, 3], dtype=torch.int32), "int64"),
                         (5, [0.1] * 16, "oks_ap")):
        a = _nms_args()
        a[i] = bad
        with pytest.raises(ValueError, match=word):
            ops._pose_rescore_nms(*a)
    with pytest.raises(ValueError, match="table position 0 has 1025 persons.*STL_POSE_NMS_MAX"):
        ops._pose_rescore_nms(*_nms_args(n=1025))
    with pytest.raises(NotImplementedError, match="CPU"):          # through the dispatcher: there is no CPU kernel
        torch.ops.stlpose.pose_rescore_nms(*_nms_args())


def _match_args(n=3, g=2, scores=None, area=None):
    return [torch.zeros(n, 17, 3, dtype=torch.float64), torch.zeros(n, dtype=torch.float64) if scores is None else scores, area,
            torch.tensor([0, n]), torch.zeros(g, 17, 3, dtype=torch.float64), torch.ones(g, dtype=torch.float64),
            torch.zeros(g, 4, dtype=torch.float64), torch.zeros(g, dtype=torch.uint8), torch.ones(g, dtype=torch.int32),
            torch.tensor([0, g]), [float(t) for t in R.OKS_THRS], [float(v) for r in R.AREA_RANGES for v in r],
            [float(s) for s in COCO_SIGMAS]]


def test_match_wrapper_refuses_before_launch():
    from stlpose_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops._oks_ap_match(*_match_args())
    for i, bad, word in ((0, torch.zeros(3, 17, 3), "float64"), (0, torch.zeros(3, 51, dtype=torch.float64), "kpts"),
                         (1, torch.zeros(3), "scores must be float64"), (2, torch.zeros(2, dtype=torch.float64), "area"),
                         (3, torch.tensor([0, 2]), "det_offsets"), (4, torch.zeros(2, 17, 2, dtype=torch.float64), "gt_kpts"),
                         (6, torch.zeros(2, 4), "gt_bbox"), (7, torch.zeros(2, dtype=torch.bool), "uint8"),
                         (8, torch.ones(2, dtype=torch.int64), "int32"), (9, torch.tensor([0, 1, 2]), "images"),
                         (10, [.5], "thresholds"), (11, [0., 1.], "area ranges"), (12, [0.1] * 16, "oks_ap")):
        a = _match_args()
        a[i] = bad
        with pytest.raises(ValueError, match=word):
            ops._oks_ap_match(*a)
    with pytest.raises(ValueError, match="STL_BOX_MAX"):
        ops._oks_ap_match(*_match_args(n=4097))
    with pytest.raises(ValueError, match="table position 0 has 129 ground truths.*STL_BOX_AP_GT_MAX"):
        ops._oks_ap_match(*_match_args(g=129))
    with pytest.raises(ValueError, match="NaN"):
        ops._oks_ap_match(*_match_args(scores=torch.tensor([.5, float("nan"), .1], dtype=torch.float64)))
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.stlpose.oks_ap_match(*_match_args())


def test_ops_are_listed_and_traceable():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from stlpose_amd import ops
    assert "pose_rescore_nms" in ops.OPS and "oks_ap_match" in ops.OPS
    assert (capi.POSE_JOINTS, capi.POSE_NMS_MAX, capi.OKS_AP_THRS, capi.OKS_AP_AREAS, capi.OKS_AP_DETS) == (17, 1024, 10, 3, 20)
    with FakeTensorMode():
        a = [torch.empty(t.shape, dtype=t.dtype, device="cuda") if isinstance(t, torch.Tensor) else t for t in _nms_args()]
        score, keep, count = torch.ops.stlpose.pose_rescore_nms(*a)
        assert score.shape == keep.shape == (3,) and count.shape == (1,) and score.dtype == torch.float64
        a = [torch.empty(t.shape, dtype=t.dtype, device="cuda") if isinstance(t, torch.Tensor) else t for t in _match_args()]
        out = torch.ops.stlpose.oks_ap_match(*a)
        assert [tuple(t.shape) for t in out] == [(3,)] * 5 + [(1, 1, 3)] and out[0].dtype == torch.float64


# ------------------------------------------------------------------------------------------------ the public functions
def test_public_functions_check_their_arguments():
    from stlpose_amd import keypoint_ap, rescore_and_nms_device
    from stlpose_amd.evaluate import Evaluator
    preds, boxes = np.zeros((1025, 17, 3), np.float32), np.zeros((1025, 6))
    with pytest.raises(ValueError, match="image_id 7: 1025 persons.*STL_POSE_NMS_MAX"):
        rescore_and_nms_device(preds, boxes, [7] * 1025, device="cpu")
    with pytest.raises(ValueError, match="float32 or float64"):
        rescore_and_nms_device(preds[:2].astype(np.float16), boxes[:2], [1, 1], device="cpu")
    with pytest.raises(ValueError, match=r"\[P, 17, 3\]"):
        rescore_and_nms_device(preds[:2, :16], boxes[:2], [1, 1], device="cpu")
    with pytest.raises(ValueError, match="image ids"):
        rescore_and_nms_device(preds[:2], boxes[:2], [1], device="cpu")
    with pytest.raises(ValueError, match="mean_order"):
        rescore_and_nms_device(preds[:2], boxes[:2], [1, 1], device="cpu", mean_order="pairwise")
    for md in (0, 21):
        with pytest.raises(ValueError, match="STL_OKS_AP_DETS"):
            keypoint_ap([], [], max_dets=md, device="cpu")
    with pytest.raises(ValueError, match="oks_ap"):
        keypoint_ap([], [], sigmas=COCO_SIGMAS[:16], device="cpu")
    with pytest.raises(ValueError, match="scoring"):
        Evaluator(None, device="cpu", scoring="gpu")
    assert Evaluator(None, device="cpu").scoring == "host"


def test_pose_results_round_trip():
    from stlpose_amd import PoseResults
    preds, boxes, ids = R.nms_set(dtype=np.float32)
    lst = rescore_and_nms(preds[:200], boxes[:200], ids[:200].tolist())
    res = PoseResults.from_list(lst, device="cpu")
    assert len(res) == len(lst) and res.keypoints.dtype == res.scores.dtype == torch.float64
    assert res.image_ids.tolist() == list(dict.fromkeys(r["image_id"] for r in lst))
    back = res.to_list()
    assert back == lst and [list(r) for r in back] == [list(r) for r in lst]          # values and key order: the same json
    assert all(type(r["image_id"]) is int and type(r["score"]) is float and type(r["keypoints"][0]) is float for r in back)
    with pytest.raises(ValueError, match="adjacent"):
        PoseResults.from_list([lst[0], lst[-1], lst[0]], device="cpu")
    assert PoseResults.from_list([], device="cpu").to_list() == []
