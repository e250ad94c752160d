"""GPU: stlpose::box_ap_match / box_ap_accumulate and stlpose_amd.detection_eval against the fp64 numpy yardstick
(tests/box_ap_ref.py).  The contract is exactness: precision and recall are compared with np.array_equal."""
import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import CocoEvaluator, DetectorEvaluator, capi, detection_eval as DE
from tests import box_ap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CATS = [1, 2, 3]            # 3 has no ground truth anywhere, 2 has ground truth and no detection; label 7 is in no list
COUNTS = [0, 1, 63, 64, 65, 100, 101, 150]


def _ragged_set():
    """40 images.  Integer and half-integer coordinates: the float32 xyxy boxes, their xywh form and every IoU below are exact."""
    rng = np.random.Generator(np.random.PCG64(2024))
    values = np.arange(1, 41, dtype=np.float32) / np.float32(64)          # 40 distinct scores: ties within and across images
    gts, preds = [], {}
    for i in range(40):
        img = 1000 + 3 * i
        n = COUNTS[i % len(COUNTS)]
        ng = 0 if i in (8, 16) else int(rng.integers(1, 9))               # image 8: no detection and no ground truth
        gb = []
        for j in range(ng):
            side = [32, 96, int(rng.integers(4, 30)), int(rng.integers(40, 90)), int(rng.integers(100, 200))][int(rng.integers(0, 5))]
            x, y = (int(v) for v in rng.integers(0, 300, 2))
            w, h = (side, side) if side in (32, 96) else (side, int(rng.integers(4, 200)))      # areas 1024 and 9216 among them
            if j > 0 and rng.random() < .2:
                x, y, w, h = gb[j - 1]                                     # a duplicated ground truth: IoU ties
            gb.append((x, y, w, h))
            gts.append(dict(image_id=img, category_id=2 if rng.random() < .15 else 1, bbox=[float(v) for v in (x, y, w, h)],
                            area=float(w * h), iscrowd=int(rng.random() < .15)))
        boxes = np.zeros((n, 4), np.float32)
        for d in range(n):
            kind = rng.integers(0, 7)
            if gb and kind < 5:
                x, y, w, h = gb[int(rng.integers(0, len(gb)))]
                if kind == 1:
                    h = h / 2                                              # IoU exactly .5 with its ground truth
                elif kind == 2:
                    h = h * 3 / 4                                          # IoU exactly .75
                elif kind == 3:
                    x, y = x + int(rng.integers(-6, 7)), y + int(rng.integers(-6, 7))
                elif kind == 4:
                    w = 0                                                  # zero width
            else:
                x, y, w, h = (int(v) for v in rng.integers(0, 300, 4))
            boxes[d] = (x, y, x + w, y + h)
        if n > 2:
            boxes[n // 2] = boxes[0]                                       # a duplicated detection
        labels = rng.choice([1, 1, 1, 1, 3, 7], n).astype(np.int32)
        if n >= 100 and i < 24:
            labels[:] = 1                                                  # exactly 100, and 101 / 150: cut at 100 per category
        preds[img] = dict(boxes=torch.from_numpy(boxes).reshape(-1, 4), labels=torch.from_numpy(labels),
                          scores=torch.from_numpy(values[rng.integers(0, 40, n)]))
    return gts, preds


def _results(preds):
    """COCO result dicts of detector outputs: xywh by a float32 subtraction, as the reference's convert_to_xywh does it."""
    out = []
    for img, p in preds.items():
        b = p["boxes"].reshape(-1, 4).float().cpu()
        xywh = torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], 1).double().tolist()
        for bb, l, s in zip(xywh, p["labels"].cpu().tolist(), p["scores"].cpu().tolist()):
            out.append(dict(image_id=int(img), category_id=int(l), bbox=bb, score=s))
    return out


@pytest.fixture(scope="module")
def ragged():
    gts, preds = _ragged_set()
    want = R.box_ap(gts, _results(preds), img_ids=list(preds), cat_ids=CATS)
    return gts, preds, want


def _evaluator(gts, preds, split=3):
    ev = CocoEvaluator(dict(annotations=gts, categories=[dict(id=c) for c in CATS]), ("bbox",))
    items = list(preds.items())[::-1]                                      # updates in descending id order, a few images each
    for i in range(0, len(items), split):
        ev.update(dict(items[i:i + split]))
    ev.synchronize_between_processes()
    return ev


def test_match_and_accumulate_equal_the_yardstick(ragged):
    gts, preds, want = ragged
    ev = _evaluator(gts, preds)
    ev.accumulate()
    got = ev.coco_eval["bbox"]
    assert got.precision.shape == (10, 101, 3, 4, 3) and got.recall.shape == (10, 3, 4, 3)
    assert (want["precision"][:, :, 0] > 0).any() and (want["recall"][:, 0] > 0).all()      # the set is not degenerate
    assert len(np.unique(want["recall"][:, 0, 0, 2])) > 3                                   # matches change with the threshold
    assert (want["precision"][:, :, 2] == -1).all()                                         # category 3: nothing to find
    assert (want["recall"][:, 1, 0] == 0).all() and (want["precision"][:, :, 1, 0] == 0).all()   # category 2: nothing found
    assert np.array_equal(got.recall, want["recall"])
    assert np.array_equal(got.precision, want["precision"])
    assert np.array_equal(ev.summarize()["bbox"], want["stats"])
    res = _results(preds)
    assert np.array_equal(stlpose_amd.box_ap(gts, res, img_ids=list(preds), cat_ids=CATS), want["stats"])
    assert np.array_equal(stlpose_amd.box_ap(gts, res[::-1], max_dets=(2, 5, 50))[[0, 8]],
                          R.box_ap(gts, res[::-1], max_dets=(2, 5, 50))["stats"][[0, 8]])


def test_match_slots(ragged):
    """The per-slot outputs: every kept detection appears once, in its category, with its rank and score."""
    gts, preds, _ = ragged
    ev = _evaluator(gts, preds)
    uniq, boxes, scores, labels, off = ev._tables
    gt = ev.gt.select(uniq)[:5]
    score, cat, rank, matched, ignored, npig = torch.ops.stlpose.box_ap_match(
        boxes, scores, labels, off, *gt, torch.tensor(CATS), [float(t) for t in R.IOU_THRS], [float(v) for r in R.AREA_RANGES for v in r])
    per_image, _, _ = R.evaluate_images(gts, _results(preds), img_ids=list(preds), cat_ids=CATS)
    cat, rank, score, matched, ignored, npig = (t.cpu().numpy() for t in (cat, rank, score, matched, ignored, npig))
    for i in range(len(uniq)):
        seg = slice(int(off[i]), int(off[i + 1]))
        for k in range(3):
            e = per_image[k][i]
            rows = np.where(cat[seg] == k)[0]
            assert len(rows) == (0 if e is None else len(e[0]["scores"]))
            if e is None:
                assert (npig[i, k] == 0).all()
                continue
            assert np.array_equal(rank[seg][rows], np.arange(len(rows)))
            assert np.array_equal(score[seg][rows].astype(np.float64), e[0]["scores"])
            for a in range(4):
                assert npig[i, k, a] == e[a]["npig"]
                for t in range(10):
                    bit = t * 4 + a
                    assert np.array_equal((matched[seg][rows] >> bit) & 1, e[a]["matched"][t].astype(np.int64))
                    assert np.array_equal((ignored[seg][rows] >> bit) & 1, e[a]["ignored"][t].astype(np.int64))
    assert (matched >> 40 == 0).all() and (ignored >> 40 == 0).all()


def test_accumulate_alone_at_the_scan_tile():
    """Synthetic matches; per category 1023, 1024, 1025 and 3000 slots (one below, at, one above the scan tile, three tiles),
    none with ground truth to find, and none at all."""
    tile = capi.BOX_AP_SCAN_TILE
    sizes = [tile - 1, tile, tile + 1, 3000, 0, 40]
    rng = np.random.Generator(np.random.PCG64(7))
    per_image, flat = [], dict(m=[], i=[], r=[], s=[], c=[])
    for k, total in enumerate(sizes):
        row, left = [], total
        while left > 0 or not row:
            d = min(left, int(rng.choice([100, 100, 37, 1, 12])))
            sc = np.sort(rng.integers(1, 9, d).astype(np.float64) / 8)[::-1]
            e = []
            for a in range(4):
                e.append(dict(scores=sc, matched=rng.random((10, d)) < .6, ignored=rng.random((10, d)) < .2,
                              npig=0 if k == 5 else int(rng.integers(1, 4))))
            row.append(e)
            bits = lambda key: sum((e[a][key][t].astype(np.int64) << (t * 4 + a)) for a in range(4) for t in range(10))
            flat["m"].append(bits("matched") if d else np.zeros(0, np.int64)), flat["i"].append(bits("ignored") if d else np.zeros(0, np.int64))
            flat["r"].append(np.arange(d, dtype=np.int32)), flat["s"].append(sc), flat["c"].append(np.full(d, k))
            left -= d
        per_image.append(row)
    want_p, want_r = R.accumulate(per_image)
    m, i, r, s, c = (np.concatenate(flat[key]) for key in "mirsc")
    order, cat_offsets = [], [0]
    for k in range(len(sizes)):
        rows = np.where(c == k)[0]
        order.append(rows[np.argsort(-s[rows], kind="mergesort")])
        cat_offsets.append(cat_offsets[-1] + len(rows))
    npig = np.array([[sum(e[a]["npig"] for e in row) for a in range(4)] for row in per_image], np.int64)
    assert (npig[:5] > 0).all() and (npig[5] == 0).all()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    p, rc = torch.ops.stlpose.box_ap_accumulate(t(m), t(i), t(r), t(np.concatenate(order)), torch.tensor(cat_offsets), t(npig), 10,
                                                [1, 10, 100], [float(v) for v in R.REC_THRS])
    assert (want_p[:, :, 5] == -1).all() and (want_p[:, :, 4] == 0).all() and (want_r[:, 4] == 0).all()
    assert np.array_equal(rc.cpu().numpy(), want_r)
    assert np.array_equal(p.cpu().numpy(), want_p)


def test_two_runs_are_bitwise_equal(ragged):
    gts, preds, _ = ragged
    ev = _evaluator(gts, preds, split=40)
    uniq, boxes, scores, labels, off = ev._tables
    gt = ev.gt.select(uniq)[:5]
    args = (boxes, scores, labels, off, *gt, torch.tensor(CATS), [float(t) for t in R.IOU_THRS], [float(v) for r in R.AREA_RANGES for v in r])
    a, b = torch.ops.stlpose.box_ap_match(*args), torch.ops.stlpose.box_ap_match(*args)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    pa, pb = (DE.evaluate_tables(boxes, scores, labels, off, gt, CATS) for _ in range(2))
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])


def test_caps_raise():
    gt = [dict(image_id=1, category_id=1, bbox=[0., 0., 10., 10.], area=100., iscrowd=0)]
    n = capi.BOX_MAX + 1
    with pytest.raises(ValueError, match="image_id 1: .*position 0 has 4097 detections.*STL_BOX_MAX"):
        stlpose_amd.box_ap(gt, [dict(image_id=1, category_id=1, bbox=[0., 0., 10., 10.], score=.5)] * n)
    with pytest.raises(ValueError, match="image_id 5: .*position 1 has 129 ground truths of category 1.*STL_BOX_AP_GT_MAX"):
        stlpose_amd.box_ap([dict(gt[0], image_id=0, category_id=2)] + [dict(g, image_id=5) for g in gt * (capi.BOX_AP_GT_MAX + 1)],
                           [dict(image_id=5, category_id=1, bbox=[0., 0., 10., 10.], score=.5)])
    ev = CocoEvaluator(gt)
    ev.update({1: dict(boxes=torch.zeros(1, 4), labels=torch.ones(1), scores=torch.tensor([float("nan")]))})
    with pytest.raises(ValueError, match="NaN"):
        ev.accumulate()
    # exactly at the caps it runs
    s = stlpose_amd.box_ap(gt * capi.BOX_AP_GT_MAX, [dict(image_id=1, category_id=1, bbox=[0., 0., 10., 10.], score=.5)] * capi.BOX_MAX)
    assert s[8] == 100 / capi.BOX_AP_GT_MAX     # AR@100: the first 100 detections each find one of the 128 identical boxes


def test_detector_evaluator_end_to_end():
    """D0 with seeded random weights at batch 2, the threshold lowered until detections exist: DetectorEvaluator's numbers equal
    the yardstick fed the same model() outputs."""
    torch.manual_seed(0)
    model = stlpose_amd.setup_detector("efficientdet", "d0", num_classes=2).to(DEV)
    imgs = torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(1)) * 255
    _, _, cls, _ = model(imgs.to(DEV) / 255, postprocess=False)
    model.threshold = float(torch.topk(cls.amax(2).flatten(), 200).values[-1])
    outputs = model(imgs.to(DEV) / 255)
    assert sum(len(o["scores"]) for o in outputs) >= 4
    ids = [11, 4]
    gts = []
    for img, o in zip(ids, outputs):            # ground truth from a few detections, shifted: matches at some thresholds only
        for j in range(0, min(len(o["scores"]), 12), 3):
            x1, y1, x2, y2 = (float(v) for v in o["boxes"][j])
            gts.append(dict(image_id=img, category_id=int(o["labels"][j]), bbox=[x1 + 1.5, y1, x2 - x1, (y2 - y1) * .9],
                            area=(x2 - x1) * (y2 - y1) * .9, iscrowd=int(j == 6)))
    loader = [([imgs[0], imgs[1]], [dict(image_id=torch.tensor(ids[0])), dict(image_id=ids[1])])]
    got = DetectorEvaluator(model).evaluate(loader, gts)
    want = R.box_ap(gts, _results(dict(zip(ids, outputs))), img_ids=ids)
    assert (want["stats"][[0, 8]] > 0).all()
    assert np.array_equal(got["stats"], want["stats"]) and got["valid_ap"] == want["stats"][0]
    skipped = DetectorEvaluator(model).evaluate(loader * 5, gts, fraction=0.2)      # the first fifth: that one batch
    assert np.array_equal(skipped["stats"], want["stats"])
