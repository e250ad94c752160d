"""CPU: the box AP yardstick (tests/box_ap_ref.py) pinned by hand-computed cases, and the host side of
stlpose_amd.detection_eval: table packing, duplicate image ids, the one-rank gather and the ops' argument checks.
pycocotools is not installed: the expected numbers below are worked out by hand from the published algorithm."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import box_ap_ref as R

AP, AP50, AP75, APS, APM, APL, AR1, AR10, AR100, ARS, ARM, ARL = range(12)


def near(x, v):
    """precision is tp / (fp + tp + 2^-52): one true positive alone gives 1 - 2^-52, not 1.  Recall is exact."""
    return bool(np.all(np.abs(np.asarray(x, np.float64) - v) < 1e-12))


def _gt(img, box, cat=1, crowd=0, area=None):
    return dict(image_id=img, category_id=cat, bbox=list(box), area=box[2] * box[3] if area is None else area, iscrowd=crowd)


def _dt(img, box, score, cat=1):
    return dict(image_id=img, category_id=cat, bbox=list(box), score=score)


# ---------------------------------------------------------------------------------------------- the yardstick
def test_thresholds_are_the_published_ones():
    assert R.IOU_THRS[0] == .5 and R.IOU_THRS[5] == .75 and len(R.IOU_THRS) == 10
    assert np.array_equal(R.REC_THRS, np.linspace(0, 1, 101)) and R.REC_THRS[50] == .5
    assert R.AREA_RANGES == [(0, 1e10), (0, 1024), (1024, 9216), (9216, 1e10)]


def test_perfect_detections_and_area_split():
    boxes = [(0, 0, 10, 10), (100, 100, 120, 110)]          # one small (100), one large (13200); nothing medium
    gts = [_gt(1, b) for b in boxes]
    dts = [_dt(1, b, s) for b, s in zip(boxes, (.9, .8))]
    s = R.box_ap(gts, dts)["stats"]
    assert near(s[[AP, AP50, AP75, APS, APL]], 1) and s[APM] == -1
    assert s[AR1] == .5 and s[AR10] == s[AR100] == 1          # the top detection alone finds one of the two
    assert s[ARS] == 1 and s[ARL] == 1 and s[ARM] == -1


def test_one_of_two_found_is_51_recall_points():
    gts = [_gt(1, (0, 0, 50, 50)), _gt(1, (200, 200, 50, 50))]
    out = R.box_ap(gts, [_dt(1, (0, 0, 50, 50), .9)])
    # recall reaches .5: precision 1 at the 51 recall points 0, .01, ..., .50 and 0 behind them
    assert near(out["precision"][0, :, 0, 0, 2], (np.arange(101) <= 50).astype(float))
    assert near(out["stats"][AP], 51 / 101) and out["stats"][AR100] == .5


def test_iou_exactly_on_a_threshold():
    assert R.bb_iou([0, 0, 10, 5], [0, 0, 10, 10], False) == .5
    out = R.box_ap([_gt(1, (0, 0, 10, 10))], [_dt(1, (0, 0, 10, 5), .9)])
    assert np.array_equal(out["recall"][:, 0, 0, 2], [1] + [0] * 9)   # counts at t = .50, not at .55
    assert near(out["stats"][AP50], 1) and out["stats"][AP75] == 0 and near(out["stats"][AP], .1)


def test_crowd_absorbs_detections():
    gts = [_gt(1, (0, 0, 40, 40)), _gt(1, (100, 100, 200, 200), crowd=1)]
    dts = [_dt(1, (110, 110, 30, 30), .95), _dt(1, (150, 150, 30, 30), .9), _dt(1, (200, 200, 30, 30), .85), _dt(1, (0, 0, 40, 40), .5)]
    assert R.bb_iou(dts[0]["bbox"], gts[1]["bbox"], True) == 1.0    # crowd: intersection over the detection's own area
    s = R.box_ap(gts, dts)["stats"]
    assert near(s[AP], 1) and s[AR100] == 1                          # three better-scored detections, none a false positive
    gts[1]["iscrowd"] = 0
    assert R.box_ap(gts, dts)["stats"][AP] < .3                      # as a regular ground truth two of them are


def test_area_boundaries_belong_to_both_ranges():
    s = R.box_ap([_gt(1, (0, 0, 32, 32))], [_dt(1, (0, 0, 32, 32), .9)])["stats"]       # area 1024
    assert near(s[[APS, APM]], 1) and s[APL] == -1
    s = R.box_ap([_gt(1, (0, 0, 96, 96))], [_dt(1, (0, 0, 96, 96), .9)])["stats"]       # area 9216
    assert s[APS] == -1 and near(s[[APM, APL]], 1)


def test_unmatched_detection_outside_the_range_is_ignored():
    gts = [_gt(1, (0, 0, 10, 10))]
    dts = [_dt(1, (300, 300, 200, 200), .9), _dt(1, (0, 0, 10, 10), .5)]
    s = R.box_ap(gts, dts)["stats"]
    assert near(s[APS], 1)                              # the large false positive does not count among the small
    assert near(s[AP], .5)                              # over all areas it does: 1 / (1 + 1 + 2^-52)


def test_category_without_ground_truth_is_minus_one():
    gts = [_gt(1, (0, 0, 50, 50), cat=1)]
    dts = [_dt(1, (0, 0, 50, 50), .9, cat=1), _dt(1, (0, 0, 50, 50), .8, cat=2)]
    out = R.box_ap(gts, dts)
    assert out["precision"].shape == (10, 101, 2, 4, 3)
    assert (out["precision"][:, :, 1] == -1).all() and (out["recall"][:, 1] == -1).all()
    assert near(out["stats"][AP], 1)


def test_max_dets_one_keeps_the_top_detection_per_image():
    boxes = [(0, 0, 50, 50), (200, 200, 50, 50)]
    out = R.box_ap([_gt(1, b) for b in boxes] + [_gt(2, boxes[0])],
                   [_dt(1, boxes[0], .9), _dt(1, boxes[1], .8), _dt(2, boxes[0], .7)])
    assert near(out["stats"][AR1], 2 / 3) and out["stats"][AR10] == 1    # image 1: the better one of its 2, image 2: 1 of 1
    assert near(out["precision"][0, :, 0, 0, 0], (np.arange(101) <= 66).astype(float))   # recall 2/3: points 0 .. .66


def test_equal_scores_keep_input_order():
    gts = [_gt(1, (0, 0, 50, 50))]
    miss, hit = _dt(1, (300, 300, 50, 50), .5), _dt(1, (0, 0, 50, 50), .5)
    assert near(R.box_ap(gts, [hit, miss])["stats"][AP], 1)
    assert near(R.box_ap(gts, [miss, hit])["stats"][AP], .5)


def test_tie_in_iou_moves_to_the_later_ground_truth():
    gts = [_gt(1, (0, 0, 50, 50)), _gt(1, (0, 0, 50, 50))]
    e = R.evaluate_image(gts, [_dt(1, (0, 0, 50, 50), .9)])
    assert e[0]["matched"][:, 0].all() and e[0]["npig"] == 2


# ---------------------------------------------------------------------------------------------- host side of the package
def _predictions():
    b1 = torch.tensor([[10.25, 20.5, 110.75, 220.125], [0.1, 0.2, 0.3, 0.7]])
    return {7: dict(boxes=b1, labels=torch.tensor([1, 2], dtype=torch.int32), scores=torch.tensor([.9, .8])),
            3: dict(boxes=torch.zeros(0), labels=torch.zeros(0, dtype=torch.int32), scores=torch.zeros(0)),
            5: dict(boxes=torch.tensor([[1., 2., 4., 8.]]), labels=torch.tensor([1]), scores=torch.tensor([.5]))}


def test_update_packs_xyxy_as_xywh():
    from stlpose_amd import CocoEvaluator
    ev = CocoEvaluator([_gt(7, (0, 0, 10, 10))], ("bbox",), device="cpu")
    p = _predictions()
    ev.update(p)
    ids, cnt, boxes, scores, labels = ev._chunks[0]
    assert ids.tolist() == [7, 3, 5] and cnt.tolist() == [2, 0, 1]
    b = p[7]["boxes"]
    want = torch.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)    # the subtraction in float32, then widened
    assert boxes.dtype == torch.float64 and torch.equal(boxes[:2], want.double()) and boxes[2].tolist() == [1, 2, 3, 6]
    assert scores.dtype == torch.float32 and labels.dtype == torch.int64 and labels.tolist() == [1, 2, 1]
    ev.synchronize_between_processes()
    uniq, tb, ts, tl, off = ev._tables
    assert uniq.tolist() == [3, 5, 7] and off.tolist() == [0, 0, 1, 3] and ev.img_ids == [3, 5, 7]
    assert tb[0].tolist() == [1, 2, 3, 6] and torch.equal(tb[1:], want.double()) and tl.tolist() == [1, 1, 2]


def test_duplicate_image_ids_count_once_first_occurrence():
    from stlpose_amd import CocoEvaluator
    ev = CocoEvaluator([_gt(7, (0, 0, 10, 10))], device="cpu")
    ev.update(_predictions())
    ev.update({5: dict(boxes=torch.tensor([[0., 0., 9., 9.], [1., 1., 2., 2.]]), labels=torch.tensor([4, 4]), scores=torch.tensor([.1, .2])),
               9: dict(boxes=torch.tensor([[0., 0., 5., 5.]]), labels=torch.tensor([3]), scores=torch.tensor([.3]))})
    ev.synchronize_between_processes()
    uniq, tb, ts, tl, off = ev._tables
    assert uniq.tolist() == [3, 5, 7, 9] and off.tolist() == [0, 0, 1, 3, 4]
    assert tl.tolist() == [1, 1, 2, 3] and tb[0].tolist() == [1, 2, 3, 6]      # image 5 as the first update gave it


def test_one_rank_gloo_group_gives_the_same_tables():
    import torch.distributed as dist
    from stlpose_amd import CocoEvaluator
    evs = [CocoEvaluator([_gt(7, (0, 0, 10, 10))], device="cpu") for _ in range(2)]
    for ev in evs:
        ev.update(_predictions())
        ev.update({5: dict(boxes=torch.tensor([[0., 0., 9., 9.]]), labels=torch.tensor([4]), scores=torch.tensor([.1]))})
    evs[0].synchronize_between_processes()
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "rendezvous"), rank=0, world_size=1)
        try:
            evs[1].synchronize_between_processes(dist.group.WORLD)
        finally:
            dist.destroy_process_group()
    for a, b in zip(evs[0]._tables, evs[1]._tables):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.asarray(a).dtype == np.asarray(b).dtype


def test_ground_truth_sources_and_iou_types(tmp_path):
    import json
    from stlpose_amd import CocoEvaluator
    anns = [_gt(2, (0, 0, 10, 10), cat=3), _gt(1, (5, 5, 10, 10), cat=1), _gt(2, (1, 1, 2, 2), cat=1, crowd=1)]
    ds = dict(annotations=anns, categories=[dict(id=1), dict(id=3), dict(id=8)], images=[])
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(ds))

    class Coco:
        dataset = ds
    a, b, c = (CocoEvaluator(src, device="cpu").gt for src in (anns, str(path), Coco()))
    assert a.cat_ids is None and b.cat_ids == c.cat_ids == [1, 3, 8]
    for g in (a, b, c):
        assert g.img_ids.tolist() == [1, 2] and g.labels.tolist() == [1, 3, 1] and g.crowd.tolist() == [0, 0, 1]
        box, area, lab, crowd, off, _ = g.select(np.array([0, 2, 5]))
        assert off.tolist() == [0, 0, 2, 2] and lab.tolist() == [3, 1] and area.tolist() == [100, 4]
    for bad in ("keypoints", "segm"):
        with pytest.raises(NotImplementedError, match="oks_ap"):
            CocoEvaluator(anns, ("bbox", bad), device="cpu")


def _match_args(n=3, g=2, scores=None):
    return [torch.zeros(n, 4, dtype=torch.float64), torch.zeros(n) if scores is None else scores, torch.ones(n, dtype=torch.int64),
            torch.tensor([0, n]), torch.zeros(g, 4, dtype=torch.float64), torch.ones(g, dtype=torch.float64),
            torch.ones(g, dtype=torch.int64), torch.zeros(g, dtype=torch.uint8), torch.tensor([0, g]), torch.tensor([1, 2]),
            [float(t) for t in R.IOU_THRS], [float(v) for r in R.AREA_RANGES for v in r]]


def test_match_wrapper_refuses_before_launch():
    from stlpose_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops._box_ap_match(*_match_args())
    for i, bad, word in ((0, torch.zeros(3, 4), "float64"), (1, torch.zeros(3, dtype=torch.float64), "float32"),
                         (2, torch.ones(3, dtype=torch.int32), "int64"), (3, torch.tensor([0, 2]), "det_offsets"),
                         (7, torch.zeros(2, dtype=torch.bool), "uint8"), (8, torch.tensor([0, 1, 2]), "images"),
                         (9, torch.tensor([2, 1]), "ascending"), (10, [.5], "thresholds")):
        a = _match_args()
        a[i] = bad
        with pytest.raises(ValueError, match=word):
            ops._box_ap_match(*a)
    with pytest.raises(ValueError, match="STL_BOX_MAX"):
        ops._box_ap_match(*_match_args(n=4097))
    with pytest.raises(ValueError, match="table position 0 has 129 ground truths of category 1.*STL_BOX_AP_GT_MAX"):
        ops._box_ap_match(*_match_args(g=129))
    with pytest.raises(ValueError, match="NaN"):
        ops._box_ap_match(*_match_args(scores=torch.tensor([.5, float("nan"), .1])))
    with pytest.raises(NotImplementedError, match="CPU"):          # through the dispatcher: there is no CPU kernel
        torch.ops.stlpose.box_ap_match(*_match_args())


def _acc_args(s=5, k=2):
    return [torch.zeros(s, dtype=torch.int64), torch.zeros(s, dtype=torch.int64), torch.zeros(s, dtype=torch.int32),
            torch.arange(s), torch.tensor([0, 2, s][:k + 1]), torch.ones(k, 4, dtype=torch.int64), 10, [1, 10, 100],
            [float(r) for r in R.REC_THRS]]


def test_accumulate_wrapper_refuses_before_launch():
    from stlpose_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops._box_ap_accumulate(*_acc_args())
    for i, bad, word in ((0, torch.zeros(5, dtype=torch.int32), "int64"), (2, torch.zeros(5, dtype=torch.int64), "int32"),
                         (3, torch.arange(4), "order"), (4, torch.tensor([0, 6, 5]), "cat_offsets"),
                         (4, torch.tensor([0, 5]), "cat_offsets"), (5, torch.ones(2, 4, dtype=torch.int32), "npig"),
                         (6, 17, "64 bits"), (7, list(range(1, 10)), "STL_BOX_AP_MAXDETS_MAX"),
                         (8, [i / 200 for i in range(201)], "STL_BOX_AP_RECS_MAX"), (8, [.1, .2], "rise from 0"),
                         (8, [0., float("nan"), 1.], "rise from 0")):
        a = _acc_args()
        a[i] = bad
        with pytest.raises(ValueError, match=word):
            ops._box_ap_accumulate(*a)


def test_ops_are_listed_and_traceable():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from stlpose_amd import ops
    assert "box_ap_match" in ops.OPS and "box_ap_accumulate" in ops.OPS
    with FakeTensorMode():
        a = [torch.empty(t.shape, dtype=t.dtype, device="cuda") if isinstance(t, torch.Tensor) else t for t in _match_args()]
        out = torch.ops.stlpose.box_ap_match(*a)
        assert [tuple(t.shape) for t in out] == [(3,)] * 5 + [(1, 2, 4)]
        a = [torch.empty(t.shape, dtype=t.dtype, device="cuda") if isinstance(t, torch.Tensor) else t for t in _acc_args()]
        p, r = torch.ops.stlpose.box_ap_accumulate(*a)
        assert p.shape == (10, 101, 2, 4, 3) and r.shape == (10, 2, 4, 3) and p.dtype == torch.float64


def test_box_ap_checks_max_dets():
    from stlpose_amd import box_ap
    with pytest.raises(ValueError, match="STL_BOX_AP_DETS"):
        box_ap([], [], max_dets=(1, 10, 200), device="cpu")


def test_detector_evaluator_shards_an_indexable_loader():
    from stlpose_amd import DetectorEvaluator

    class Loader(list):
        touched = []

        def __getitem__(self, i):
            self.touched.append(i)
            return list.__getitem__(self, i)
    ev = DetectorEvaluator(None, device="cpu")
    ev.rank, ev.world = 1, 3
    loader = Loader(range(10))
    assert list(ev._my_batches(loader, None)) == [1, 4, 7] and loader.touched == [1, 4, 7]
    assert list(ev._my_batches(loader, 5)) == [1, 4]
    assert list(ev._my_batches(iter(range(10)), 5)) == [1, 4]          # a plain iterable is skipped through
    ev.rank, ev.world = 0, 1
    assert list(ev._my_batches(loader, 2)) == [0, 1] and list(ev._my_batches(loader, None)) == list(range(10))
