"""GPU: the detector's device tail (csrc/detections.hip, stlpose_amd/detections.py) against the host path it restates, run in the same
test: det_decode + torch.sort(stable) + det_nms + invert_affine (efficientdet.detect_from_heads / EfficientDetBackbone.detect, pinned by
fixture G15 in test_detector_gpu.py).  Every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import CocoEvaluator, DetectorEvaluator, capi, efficientdet as E
from stlpose_amd.detections import Detections, DetectionStore
from tests import detector_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "detector", "g15_effdet.npz")
DEV = "cuda"
A, THR, IOU = 6000, 0.5, 0.5
K = capi.BOX_MAX
SIZES = [(300, 420), (480, 270), (333, 517), (512, 512)]   # (h, w): landscape, portrait, landscape, identity
# one edge per image: the candidate count, or a named construction of _heads
BATCHES = [[0, 1, 64, 65], [1025, K, "ties", "twins"], ["threshold", K + 1, 37, "argmax"]]
PAIRS = 200            # the pairs of "threshold" and of "twins"
P0 = 1000              # "threshold": anchors P0 + 2k and P0 + 2k + 1 are a box and its upper half


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _anchors():
    """[A, 4] (y1, x1, y2, x2) on the 512 canvas.  Anchors 2k + 1 = 2k for k < PAIRS ("twins": identical boxes); P0 ..: PAIRS
    pairs (box, its upper half), whose IoU is 1/2 up to the rounding of the fp32 arithmetic."""
    rng = np.random.default_rng(7)
    cy, cx = rng.uniform(20, 490, A), rng.uniform(20, 490, A)
    h, w = rng.uniform(8, 160, A), rng.uniform(8, 160, A)
    an = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(np.float32)
    an[1:2 * PAIRS:2] = an[0:2 * PAIRS:2]
    for k in range(PAIRS):
        y1, x1 = rng.uniform(5, 300, 2)
        hh, ww = rng.uniform(20, 200, 2)
        if k % 4 == 0:   # integer boxes: the IoU is exactly 1/2, not above it
            y1, x1, hh, ww = float(int(y1)), float(int(x1)), float(2 * int(hh / 2)), float(int(ww))
        an[P0 + 2 * k] = (y1, x1, y1 + hh, x1 + ww)
        an[P0 + 2 * k + 1] = (y1, x1, y1 + hh / 2, x1 + ww)
    return an


def _heads(case, nc, rng):
    """reg [A, 4] and cls [A, nc] of one image."""
    reg = (rng.standard_normal((A, 4)) * 0.2).astype(np.float32)
    cls = (rng.uniform(0, 0.4, (A, nc))).astype(np.float32)
    if isinstance(case, int):
        idx = rng.choice(A, case, replace=False)
        best = rng.uniform(0.5001, 1.0, case).astype(np.float32)
    elif case == "ties":          # 300 candidates over 8 score values: the order within a group is the anchor order
        idx = rng.choice(A, 300, replace=False)
        best = rng.choice(np.linspace(0.55, 0.9, 8).astype(np.float32), 300)
    elif case == "argmax":        # the maximum twice in a row: the class is the first
        idx = rng.choice(A, 150, replace=False)
        best = rng.uniform(0.5001, 1.0, 150).astype(np.float32)
    elif case == "twins":         # identical boxes, equal scores within a pair, classes 0 and 1 (nc = 1: one class)
        idx = np.arange(2 * PAIRS)
        reg[1:2 * PAIRS:2] = reg[0:2 * PAIRS:2]
        best = np.repeat(rng.uniform(0.5001, 1.0, PAIRS).astype(np.float32), 2)
    else:                         # "threshold": undistorted anchors, so that the pairs' IoU is the constructed one
        idx = np.arange(P0, P0 + 2 * PAIRS)
        reg[idx] = 0
        best = rng.uniform(0.5001, 1.0, 2 * PAIRS).astype(np.float32)
    c = rng.integers(0, nc, len(idx))
    if case == "twins":
        c = np.arange(len(idx)) % min(nc, 2)
    if case == "threshold":
        c = np.repeat(rng.integers(0, nc, PAIRS), 2)   # a pair shares its class
    cls[idx, c] = best
    if case == "argmax" and nc > 1:
        c2 = (c + 1) % nc
        cls[idx, c2] = best
    return reg, cls


@pytest.fixture(scope="module")
def anchors():
    return torch.from_numpy(_anchors()).to(DEV)


def _batch(cases, nc, seed):
    rng = np.random.default_rng(seed)
    rc = [_heads(c, nc, rng) for c in cases]
    return torch.from_numpy(np.stack([r for r, _ in rc])).to(DEV), torch.from_numpy(np.stack([c for _, c in rc])).to(DEV)


def _records(metas):
    recs = (capi.DetImage * len(metas))()
    for i, (new_w, new_h, old_w, old_h, *_) in enumerate(metas):
        recs[i] = capi.DetImage(None, 1, old_h, old_w, new_h, new_w, 0, 1.0 / (new_h / old_h), 1.0 / (new_w / old_w))
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)


def _host(reg, cls, an, metas=None, thr=THR):
    """The existing path: per image (boxes, labels int32, scores) as numpy arrays."""
    out = []
    for i, (b, c, s) in enumerate(E.detect_from_heads(reg, cls, an, thr, IOU)):
        if metas is not None and len(s):
            b = E.invert_affine(metas[i], b)
        out.append((b, c.astype(np.int32) + 1, s))
    return out


def _expected_candidates(case):
    return case if isinstance(case, int) else {"ties": 300, "argmax": 150, "twins": 2 * PAIRS, "threshold": 2 * PAIRS}[case]


@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("nc", [1, 3])
def test_postprocess_equals_host_path(anchors, nc, resize):
    metas = [E.resize_meta(h, w) for h, w in SIZES] if resize else None
    for bi, cases in enumerate(BATCHES):
        reg, cls = _batch(cases, nc, 100 * nc + bi)
        want = _host(reg, cls, anchors, metas)
        boxes, scores, labels, count = torch.ops.stlpose.det_postprocess(reg, cls, anchors, _records(metas) if resize else None, THR,
                                                                         511.0, 511.0, IOU)
        assert boxes.shape == (4, K, 4) and scores.shape == (4, K) and labels.dtype == torch.int32 and count.dtype == torch.int32
        boxes, scores, labels, count = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), count.cpu().numpy()
        for i, case in enumerate(cases):
            n = int((cls[i].amax(1) > THR).sum())
            assert n == _expected_candidates(case)
            wb, wl, ws = want[i]
            if n > K:
                assert count[i] == -n - 1 == -4098
                continue
            k = int(count[i])
            assert k == len(ws), (case, k, len(ws))
            assert np.array_equal(_bits(scores[i, :k]), _bits(ws)), case
            assert np.array_equal(labels[i, :k], wl), case
            assert np.array_equal(_bits(boxes[i, :k]), _bits(wb.reshape(-1, 4))), case
            if case == "twins" and nc == 3:      # identical boxes of two classes: both survive
                first = np.lexsort((labels[i, :k], -scores[i, :k]))
                assert k >= 2 and (boxes[i, first[0]] == boxes[i, first[1]]).all() and labels[i, first[0]] != labels[i, first[1]]
            if case == "threshold":              # the test has pairs on both sides of the threshold
                assert 0 < k < n


def test_over_the_cap_names_image_and_count(anchors):
    reg, cls = _batch(BATCHES[2], 1, 5)
    dets = E.detect_on_device(reg, cls, anchors, THR, IOU)
    assert isinstance(dets, Detections) and dets.count.tolist()[1] == -4098
    with pytest.raises(ValueError, match=r"image 1 .* 4097 .*4096 \(STL_BOX_MAX\)"):
        dets.to_list()
    fine = Detections(dets.boxes[[0, 2]].contiguous(), dets.scores[[0, 2]].contiguous(), dets.labels[[0, 2]].contiguous(),
                      dets.count[[0, 2]].contiguous())
    assert [len(d["scores"]) for d in fine.to_list()] == [int(dets.count[0]), int(dets.count[2])]
    store = DetectionStore(1 << 14, DEV)
    store.append([5, 9, 2, 7], dets)
    with pytest.raises(ValueError, match=r"image id 9 has 4097 candidates"):
        store.finish()


# ------------------------------------------------------------------------------------------------ whole model
def _layout(g, cc):
    rows = bytes(g[f"d{cc}_layout"]).decode().split("\n")
    return {k: tuple(int(v) for v in s.split(",") if v) for k, s in (r.split(" ") for r in rows)}


@pytest.fixture(scope="module")
def state():
    return R.synth_state_dict(_layout(np.load(FIX), 0))


def _images():
    gen = torch.Generator().manual_seed(31)
    return [torch.rand(3, h, w, generator=gen) for h, w in SIZES[:3]]


def _same_lists(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert set(a) == set(b) == {"boxes", "labels", "scores"}
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", ["fp32", "f16"])
def test_forward_device_equals_forward(state, mode):
    m = E.setup_detector("efficientdet", "d0", compute_dtype=mode)
    m.load_state_dict(state, strict=True)
    m = m.to(DEV).eval()
    ims = _images()
    _, _, cls, _ = m(ims, postprocess=False)
    best = cls.amax(2)
    thr = float(torch.quantile(best.flatten(), 1.0 - 400.0 / best.shape[1]))
    n = (best > thr).sum(1).tolist()
    print("candidates per image", n, "threshold", thr)
    assert all(50 <= v <= 2000 for v in n)
    want = m(ims, threshold=thr)
    dets = m(ims, threshold=thr, output="device")
    assert isinstance(dets, Detections) and dets.device.type == "cuda" and len(dets) == 3
    assert sum(len(d["scores"]) for d in want) >= 3
    _same_lists(dets.to_list(), want)
    # the stacked-tensor input without preprocessing: no inverse resize
    x = torch.rand(2, 3, 512, 512, generator=torch.Generator().manual_seed(2)).to(DEV)
    _same_lists(m(x, preprocess=False, output="device").to_list(), m(x, preprocess=False))
    m.threshold = 1.01   # nothing passes: the empty dicts
    _same_lists(m(ims, output="device").to_list(), m(ims))
    with pytest.raises(ValueError, match="output"):
        m(ims, output="numpy")


# ------------------------------------------------------------------------------------------------ store
def _three_batches(anchors):
    cases = [[37, 0, 120, 64], [65, "ties", 1, 90], ["argmax", 10, 80, 200]]
    metas = [E.resize_meta(h, w) for h, w in SIZES]
    tab = _records(metas)
    out = []
    for bi, cs in enumerate(cases):
        reg, cls = _batch(cs, 3, 900 + bi)
        out.append(([100 * bi + j * 7 + 3 for j in range(4)][::-1], E.detect_on_device(reg, cls, anchors, THR, IOU, tab)))
    return out


def _gts(batches):
    gts = []
    for ids, dets in batches:
        for img, d in zip(ids, dets.to_list()):
            for j in range(0, min(len(d["scores"]), 12), 3):
                x1, y1, x2, y2 = (float(v) for v in d["boxes"][j])
                gts.append(dict(image_id=img, category_id=int(d["labels"][j]), bbox=[x1 + 1.5, y1, x2 - x1, (y2 - y1) * .9],
                                area=(x2 - x1) * (y2 - y1) * .9, iscrowd=int(j == 6)))
    return gts


def test_store_equals_dict_updates(anchors):
    batches = _three_batches(anchors)
    gt = dict(annotations=_gts(batches), categories=[dict(id=c) for c in (1, 2, 3)])
    a, b = CocoEvaluator(gt), CocoEvaluator(gt, store_capacity=4096)
    for ids, dets in batches:
        a.update(dict(zip(ids, dets.to_list())))
        b.update(ids, dets)
    a.synchronize_between_processes(), b.synchronize_between_processes()
    assert a.img_ids == b.img_ids and len(a.img_ids) == 12
    for x, y in zip(a._tables, b._tables):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else torch.equal(x, y)
    assert a._tables[2].shape[0] > 100 and (np.diff(a._tables[4].numpy()) == 0).sum() == 1   # one empty image
    a.accumulate(), b.accumulate()
    ea, eb = a.coco_eval["bbox"], b.coco_eval["bbox"]
    assert np.array_equal(ea.precision, eb.precision) and np.array_equal(ea.recall, eb.recall)
    sa, sb = a.summarize()["bbox"], b.summarize()["bbox"]
    assert np.array_equal(sa, sb) and sa.shape == (12,) and sa[0] > 0
    # store and dict updates in one evaluator: the dict updates first, then the store's batches
    c = CocoEvaluator(gt)
    c.update(batches[1][0], batches[1][1])
    c.update(dict(zip(batches[0][0], batches[0][1].to_list())))
    c.update(batches[2][0], batches[2][1])
    c.accumulate()
    assert np.array_equal(c.coco_eval["bbox"].precision, ea.precision)
    # a store below the total raises and names its capacity
    total = int(a._tables[2].shape[0])
    small = DetectionStore(total - 1, DEV)
    for ids, dets in batches:
        small.append(ids, dets)
    with pytest.raises(ValueError, match=rf"capacity of {total - 1} rows"):
        small.finish()
    exact = DetectionStore(total, DEV)
    for ids, dets in batches:
        exact.append(ids, dets)
    ids, cnt, boxes, scores, labels = exact.finish()
    assert cnt.sum() == total == boxes.shape[0] and boxes.dtype == torch.float64 and labels.dtype == torch.int64
    assert ids.tolist() == [i for b_ids, _ in batches for i in b_ids]


def test_slot_table_grows(anchors):
    from stlpose_amd import detections as D
    ids, dets = _three_batches(anchors)[0]
    store = DetectionStore(1 << 17, DEV)
    rounds = D.SLOTS0 // 4 + 2
    for r in range(rounds):
        store.append([4 * r + j for j in range(4)], dets)
    got_ids, cnt, boxes, _, _ = store.finish()
    assert got_ids.tolist() == list(range(4 * rounds)) and cnt.tolist() == dets.count.tolist() * rounds
    n = int(dets.count.sum())
    assert torch.equal(boxes[:n], boxes[(rounds - 1) * n:])


# ------------------------------------------------------------------------------------------------ no waits
def test_device_tail_never_waits(state):
    m = E.setup_detector("efficientdet", "d0")
    m.load_state_dict(state, strict=True)
    m = m.to(DEV).eval()
    dev = torch.device("cuda", torch.cuda.current_device())
    ims = [im.to(DEV) for im in _images()]
    _, _, cls, _ = m(ims, postprocess=False)
    thr = float(torch.quantile(cls.amax(2).flatten(), 1.0 - 400.0 / cls.shape[1]))
    gt = [dict(image_id=1, category_id=1, bbox=[0., 0., 10., 10.], area=100., iscrowd=0)]
    ev = CocoEvaluator(gt, store_capacity=1 << 14)
    ev.update([90, 91, 92], m(ims, threshold=thr, output="device"))   # the first use allocates the store
    torch.cuda.synchronize()

    def tail(output, batch):
        p, metas = m.run_raw(ims, 1, dev)   # the network and its input upload: outside the guarded region
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            dets = m.detect(p, metas, thr, 0.5, output=output)
            ids = [3 * batch + j for j in range(3)]
            if output == "device":
                ev.update(ids, dets)
            else:
                ev.update(dict(zip(ids, dets)))
        finally:
            torch.cuda.set_sync_debug_mode("default")

    for batch in range(3):
        tail("device", batch)
    with pytest.raises(RuntimeError, match="synchroniz"):   # the guard is live: the host tail trips it
        tail("host", 3)
    ev.synchronize_between_processes()
    assert len(ev.img_ids) == 12 and ev._tables[2].shape[0] > 12


def test_detector_evaluator_device_equals_host():
    torch.manual_seed(0)
    model = stlpose_amd.setup_detector("efficientdet", "d0", num_classes=2).to(DEV)
    imgs = torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(1)) * 255
    _, _, cls, _ = model(imgs.to(DEV) / 255, postprocess=False)
    model.threshold = float(torch.topk(cls.amax(2).flatten(), 200).values[-1])
    outputs = model(imgs.to(DEV) / 255)
    gts = []
    for img, o in zip((11, 4), outputs):
        for j in range(0, min(len(o["scores"]), 12), 3):
            x1, y1, x2, y2 = (float(v) for v in o["boxes"][j])
            gts.append(dict(image_id=img, category_id=int(o["labels"][j]), bbox=[x1 + 1.5, y1, x2 - x1, (y2 - y1) * .9],
                            area=(x2 - x1) * (y2 - y1) * .9, iscrowd=0))
    loader = [([imgs[0], imgs[1]], [dict(image_id=11), dict(image_id=4)])]
    want = DetectorEvaluator(model).evaluate(loader, gts)
    got = DetectorEvaluator(model, output="device").evaluate(loader, gts)
    assert want["stats"][0] > 0 and np.array_equal(got["stats"], want["stats"]) and got["valid_ap"] == want["valid_ap"]


# ------------------------------------------------------------------------------------------------ persons
DET_THR = 0.7


def _hand_made():
    """Three images (40, 0 and 300 rows): labels 1 .. 3 mixed, scores around DET_THR with exact hits, boxes wider than, taller
    than and exactly of the crop's aspect ratio, overlapping enough for NMS to act."""
    rng = np.random.default_rng(23)
    counts = [40, 0, 300]
    boxes, scores = np.zeros((3, K, 4), np.float32), np.zeros((3, K), np.float32)
    labels = np.zeros((3, K), np.int32)
    for i, n in enumerate(counts):
        x1, y1 = rng.uniform(0, 400, n), rng.uniform(0, 300, n)
        w, h = rng.uniform(10, 200, n), rng.uniform(10, 260, n)
        w[::5], h[::5] = 75.0, 100.0                                   # w == aspect * h: neither side is widened
        x1[::5], y1[::5] = np.round(x1[::5]), np.round(y1[::5])
        boxes[i, :n] = np.stack([x1, y1, x1 + w, y1 + h], 1)
        s = rng.uniform(0.5, 0.95, n).astype(np.float32)
        s[::7] = np.float32(DET_THR)                                   # exactly the threshold: not above it
        s[1::7] = np.nextafter(np.float32(DET_THR), np.float32(1))     # the next float32: above it
        s[2::11] = s[3::11][:len(s[2::11])] if len(s[3::11]) >= len(s[2::11]) else s[2::11]   # equal scores
        scores[i, :n] = s
        labels[i, :n] = rng.choice([1, 1, 1, 2, 3], n)
    boxes[2, 1], labels[2, 1], scores[2, 1] = boxes[2, 8], 1, 0.9      # an identical box: NMS drops one
    labels[2, 8], scores[2, 8] = 1, 0.91
    return counts, boxes, scores, labels


@pytest.mark.parametrize("nms_thr", [None, 0.5])
def test_person_rows_equal_select_boxes_and_coords2cs(nms_thr):
    from stlpose_amd.bounding_box import select_boxes
    from stlpose_amd.topdown import PoseExtractor
    counts, boxes, scores, labels = _hand_made()
    dets = Detections(*(torch.from_numpy(t).to(DEV) for t in (boxes, scores, labels, np.asarray(counts, np.int32))))
    ex = PoseExtractor(None)
    n, img, rb, rs, center, scale, minv = ex.person_rows(dets, label=1, det_thr=DET_THR, nms_thr=nms_thr)
    img, rb, rs, center, scale, minv = (t.cpu().numpy() for t in (img, rb, rs, center, scale, minv))
    bs, ss, ls = ([t[i, :c] for i, c in enumerate(counts)] for t in (boxes, scores, labels.astype(np.int64)))
    kept = select_boxes(bs, ss, ls, label=1, score_thr=float(np.float32(DET_THR)), iou_thr=-1.0 if nms_thr is None else nms_thr)
    assert [len(k) for k in kept][1] == 0 and len(kept[0]) > 5 and len(kept[2]) > 50
    assert n == sum(len(k) for k in kept) and img.tolist() == [i for i, k in enumerate(kept) for _ in k]
    wb, ws = np.concatenate([b[k] for b, k in zip(bs, kept)]), np.concatenate([s[k] for s, k in zip(ss, kept)])
    assert (ws > np.float32(DET_THR)).all() and (ws == np.nextafter(np.float32(DET_THR), np.float32(1))).any()
    if nms_thr is not None:
        assert n < sum(int(((l == 1) & (s > np.float32(DET_THR))).sum()) for l, s in zip(ls, ss))   # NMS dropped something
    assert np.array_equal(_bits(rb), _bits(wb)) and np.array_equal(_bits(rs), _bits(ws))
    wc, wsc = ex.transform.coords2cs(wb)
    assert np.array_equal(_bits(center), _bits(wc)) and np.array_equal(_bits(scale), _bits(wsc))
    # minv against the fp64 solution of TransformDetection.matrices, inverted in fp64: at most 4 x the distance of the host's
    # float32 minv from it, with a floor of 16 float32 ulps of the largest entry
    trans = ex.transform.matrices(wc, wsc)
    full = np.concatenate([trans, np.broadcast_to(np.array([0.0, 0.0, 1.0]), (n, 1, 3))], 1)
    exact = np.linalg.inv(full)[:, :2].reshape(n, 6)
    host = exact.astype(np.float32)
    floor = 16 * np.spacing(np.abs(exact).max(1).astype(np.float32)).astype(np.float64)
    tol = np.maximum(4 * np.abs(host.astype(np.float64) - exact), floor[:, None])
    err = np.abs(minv.astype(np.float64) - exact)
    print("minv: largest error / tolerance", float((err / tol).max()))
    assert (err <= tol).all()
    assert (minv[:, [1, 3]] == 0).all()


def test_person_rows_name_an_image_above_the_cap(anchors):
    from stlpose_amd.topdown import PoseExtractor
    reg, cls = _batch(BATCHES[2], 1, 5)
    dets = E.detect_on_device(reg, cls, anchors, THR, IOU)
    for nms_thr in (None, 0.5):
        with pytest.raises(ValueError, match="image 1 of the batch"):
            PoseExtractor(None).person_rows(dets, nms_thr=nms_thr)


def test_detect_poses_device_pipeline(state):
    from oracle import hrnet_ref
    from stlpose_amd import PoseHighResolutionNet
    from stlpose_amd.topdown import PoseExtractor, detect_poses
    d0 = E.setup_detector("efficientdet", "d0")
    d0.load_state_dict(state, strict=True)
    d0 = d0.to(DEV).eval()
    ref = hrnet_ref.load_synth(hrnet_ref.RefPoseNet("tiny")).eval()
    net = PoseHighResolutionNet("tiny", "fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV).eval()
    ex = PoseExtractor(net, batch=8)
    ims = R.images()
    d0.threshold = 0.5
    with pytest.raises(ValueError, match="pipeline"):
        detect_poses(d0, ex, ims, pipeline="gpu")
    for nms_thr in (None, 0.3):
        got = detect_poses(d0, ex, ims, detector_thr=0.5, nms_thr=nms_thr, pipeline="device")
        want = detect_poses(d0, ex, ims, detector_thr=0.5, nms_thr=nms_thr)
        # the existing kernels fed the device path's own person rows
        dev = torch.device("cuda", torch.cuda.current_device())
        src = [torch.from_numpy(im).to(dev) for im in ims]
        p, metas = d0.run_raw(src, 0, dev)
        n, img, _, _, center, scale, minv = ex.person_rows(d0.detect(p, metas, 0.5, d0.iou_threshold, output="device"), 1, 0.5, nms_thr)
        offs = torch.tensor([0, src[0].numel()], device=dev)[img.long()]
        hw = torch.tensor([s.shape[:2] for s in src], dtype=torch.int32, device=dev)[img.long()]
        from stlpose_amd.augment import IMAGENET_MEAN, IMAGENET_STD
        crops = torch.ops.stlpose.affine_crop(torch.cat([s.reshape(-1) for s in src]), offs, hw, minv,
                                              torch.zeros(n, dtype=torch.int32, device=dev), 256, 192,
                                              torch.tensor(IMAGENET_MEAN, device=dev), torch.tensor(IMAGENET_STD, device=dev))
        hm = ex.heatmaps(crops)
        preds, mx = torch.ops.stlpose.final_preds(hm, center, scale)
        _, cmx, cpreds = torch.ops.stlpose.heatmap_resize_argmax(hm.float(), 256, 192)
        kp, ckp = torch.cat([preds, mx], 2).cpu().numpy(), torch.cat([cpreds, cmx[..., None]], 2).cpu().numpy()
        assert n == sum(len(g["boxes"]) for g in got) and n > 0
        assert np.array_equal(np.concatenate([g["keypoints"] for g in got]), kp)
        assert np.array_equal(np.concatenate([g["crop_keypoints"] for g in got]), ckp)
        for g, w in zip(got, want):
            assert len(g["boxes"]) > 0 and set(g) == set(w)
            assert g["boxes"].dtype == w["boxes"].dtype and np.array_equal(_bits(g["boxes"]), _bits(w["boxes"]))
            assert np.array_equal(_bits(g["scores"]), _bits(w["scores"]))
            assert np.array_equal(_bits(g["center"]), _bits(w["center"])) and np.array_equal(_bits(g["scale"]), _bits(w["scale"]))
            assert g["keypoints"].shape == w["keypoints"].shape and g["crop_keypoints"].dtype == w["crop_keypoints"].dtype
            assert g["all_keypoints"].shape[1] == w["all_keypoints"].shape[1] == 4 and isinstance(g["pose_entries"], type(w["pose_entries"]))
            print("keypoints: device against host pipeline, largest difference", float(np.abs(g["keypoints"] - w["keypoints"]).max()))
