"""The yardstick of the device pose scoring (stlpose_amd/keypoint_eval.py): a numpy restatement of rescoring + OKS-NMS and of
COCOeval for "keypoints" that also returns the tables the ten numbers are read from, and the MARGINS: how close any OKS value the
algorithm compares came to what it was compared with.  The device's fp64 exp may differ from numpy's in the last bits (an OKS by
less than 1e-13), so its decisions are those computed here whenever the margins are far above that; the tests assert 1e-9.

Also the seeded data sets the CPU and GPU tests share.
"""
from collections import defaultdict

import numpy as np

from stlpose_amd.evaluate import COCO_SIGMAS

OKS_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(.0, 1.0, 101)
AREA_RANGES = ((0, 1e10), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))


# ------------------------------------------------------------------------------------------------ rescoring + OKS-NMS
def nms_oks_rows(kept: np.ndarray, cands: np.ndarray, a_kept: float, a_cands: np.ndarray, sigmas=None) -> np.ndarray:
    """oks_iou (lib/nms.py:48-74) of one kept pose [17, 3] against the candidates [n, 17, 3], all 17 joints."""
    var = ((COCO_SIGMAS if sigmas is None else np.asarray(sigmas)) * 2) ** 2
    dx, dy = cands[:, :, 0] - kept[None, :, 0], cands[:, :, 1] - kept[None, :, 1]
    e = (dx ** 2 + dy ** 2) / var[None, :] / ((a_kept + a_cands) / 2 + np.spacing(1))[:, None] / 2
    return np.sum(np.exp(-e), axis=1) / e.shape[1]


def rescore_nms_ref(all_preds, all_boxes, image_ids, in_vis_thr=0.2, oks_thr=0.9, mean_order="numpy"):
    """rescore_and_nms restated: returns (per image in order of first appearance: (image id, kept input rows in NMS order),
    scores float64 [P], the NMS margin = the smallest |OKS - oks_thr| over every pair the suppression compares).
    mean_order "numpy": conf[good].mean(), as evaluate.rescore_and_nms; "reference": the running sum of lib/metrics.py:242-250."""
    all_preds, all_boxes = np.asarray(all_preds), np.asarray(all_boxes, np.float64)
    conf = all_preds[:, :, 2]
    scores = np.zeros(len(all_preds))
    for p in range(len(all_preds)):
        good = conf[p] > in_vis_thr
        if mean_order == "reference":
            k, n = 0, 0
            for v in conf[p]:                       # numpy scalars of the input's dtype, as in the reference's loop
                if v > in_vis_thr:
                    k, n = k + v, n + 1
            k = float(k / n) if n else 0.0
        else:
            k = float(conf[p][good].mean()) if good.any() else 0.0
        scores[p] = k * float(all_boxes[p, 5])
    rows_of = defaultdict(list)
    for p, im in enumerate(image_ids):
        rows_of[int(im)].append(p)
    kp = all_preds.astype(np.float64)
    out, margin = [], np.inf
    for im, rows in rows_of.items():
        rows = np.asarray(rows)
        order = rows[scores[rows].argsort()[::-1]]
        keep = []
        while order.size:
            i = order[0]
            keep.append(int(i))
            rest = order[1:]
            ov = nms_oks_rows(kp[i], kp[rest], all_boxes[i, 4], all_boxes[rest, 4])
            if ov.size:
                margin = min(margin, float(np.abs(ov - oks_thr).min()))
            order = rest[ov <= oks_thr]
        out.append((im, keep))
    return out, scores, margin


# ------------------------------------------------------------------------------------------------ keypoint AP
def oks_tile(dts, gts, sigmas):
    """COCOeval.computeOks: [detections, ground truths]."""
    out = np.zeros((len(dts), len(gts)))
    if not dts or not gts:
        return out
    var = (sigmas * 2) ** 2
    d = np.asarray([dt["keypoints"] for dt in dts], np.float64).reshape(len(dts), -1, 3)
    xd, yd = d[:, :, 0], d[:, :, 1]
    for j, gt in enumerate(gts):
        g = np.asarray(gt["keypoints"], np.float64).reshape(-1, 3)
        vis = g[:, 2] > 0
        if vis.any():
            dx, dy = xd - g[None, :, 0], yd - g[None, :, 1]
        else:
            bb = gt["bbox"]
            x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
            dx = np.maximum(0.0, x0 - xd) + np.maximum(0.0, xd - x1)
            dy = np.maximum(0.0, y0 - yd) + np.maximum(0.0, yd - y1)
        e = (dx ** 2 + dy ** 2) / var[None, :] / (gt["area"] + np.spacing(1)) / 2
        if vis.any():
            e = np.ascontiguousarray(e[:, vis])
        out[:, j] = np.sum(np.exp(-e), axis=1) / e.shape[1]
    return out


def _tile_margin(oks: np.ndarray) -> float:
    """The smallest |OKS - threshold| over the tile and the ten thresholds, and the smallest non-zero gap between two entries of
    one detection's row that can both be a best match (>= 0.5 - 1e-9: entries below every threshold never are, and their mutual
    gaps go down to 1e-300)."""
    if oks.size == 0:
        return np.inf
    thr = np.minimum(OKS_THRS, 1 - 1e-10)
    m = float(np.abs(oks[:, :, None] - thr[None, None, :]).min())
    for row in oks:
        v = np.sort(row[row >= 0.5 - 1e-9])
        gaps = np.diff(v)
        gaps = gaps[gaps > 0]
        if gaps.size:
            m = min(m, float(gaps.min()))
    return m


def keypoint_ap_ref(gt_annotations, results, img_ids=None, sigmas=None, max_dets=20):
    """oks_ap restated.  Returns dict(precision [10, 101, 3], recall [10, 3], stats [10], margin)."""
    sigmas = COCO_SIGMAS if sigmas is None else np.asarray(sigmas)
    T, R, A = len(OKS_THRS), len(REC_THRS), len(AREA_RANGES)
    gt_by, dt_by = defaultdict(list), defaultdict(list)
    for a in gt_annotations:
        gt_by[a["image_id"]].append(a)
    for r in results:
        d = dict(r)
        if "area" not in d:
            k = np.asarray(d["keypoints"], np.float64).reshape(-1, 3)
            d["area"] = float((k[:, 0].max() - k[:, 0].min()) * (k[:, 1].max() - k[:, 1].min()))
        dt_by[d["image_id"]].append(d)
    ids = sorted(set(gt_by) | set(dt_by)) if img_ids is None else sorted(set(img_ids))
    margin = np.inf
    matched = [[] for _ in range(A)]     # per area range: per image [T, D] bool
    ignored = [[] for _ in range(A)]
    scores, npig = [], np.zeros(A, int)
    for im in ids:
        gts, dts = gt_by.get(im, []), dt_by.get(im, [])
        dts = [dts[i] for i in np.argsort([-d["score"] for d in dts], kind="mergesort")[:max_dets]]
        oks = oks_tile(dts, gts, sigmas)
        margin = min(margin, _tile_margin(oks))
        scores.append(np.asarray([d["score"] for d in dts], np.float64))
        crowd = np.asarray([bool(g.get("iscrowd", 0)) for g in gts], bool)
        darea = np.asarray([d["area"] for d in dts], np.float64)
        for ai, (lo, hi) in enumerate(AREA_RANGES):
            gig = np.asarray([bool(g.get("iscrowd", 0)) or g.get("num_keypoints", 1) == 0 or g["area"] < lo or g["area"] > hi
                              for g in gts], bool)
            gorder = np.argsort(gig, kind="mergesort")          # the regular ones first, stable
            nreg = int(np.count_nonzero(~gig))
            npig[ai] += nreg
            mt = np.zeros((T, len(dts)), bool)
            ig = np.zeros((T, len(dts)), bool)
            for ti, t in enumerate(OKS_THRS):
                taken = np.zeros(len(gts), bool)
                for di in range(len(dts)):
                    best, m = min(t, 1 - 1e-10), -1
                    for pos, gi in enumerate(gorder):
                        if taken[pos] and not crowd[gi]:
                            continue
                        if m > -1 and m < nreg and pos >= nreg:
                            break
                        if oks[di, gi] < best:
                            continue
                        best, m = oks[di, gi], pos
                    if m > -1:
                        mt[ti, di], ig[ti, di], taken[m] = True, m >= nreg, True
                    else:
                        ig[ti, di] = darea[di] < lo or darea[di] > hi
            matched[ai].append(mt), ignored[ai].append(ig)
    sc = np.concatenate(scores) if scores else np.zeros(0)
    order = np.argsort(-sc, kind="mergesort")
    precision, recall = -np.ones((T, R, A)), -np.ones((T, A))
    for ai in range(A):
        if npig[ai] == 0:
            continue
        mt = np.concatenate(matched[ai], axis=1)[:, order] if matched[ai] else np.zeros((T, 0), bool)
        ig = np.concatenate(ignored[ai], axis=1)[:, order] if ignored[ai] else np.zeros((T, 0), bool)
        tp = np.cumsum(mt & ~ig, axis=1).astype(float)
        fp = np.cumsum(~mt & ~ig, axis=1).astype(float)
        for ti in range(T):
            rc = tp[ti] / npig[ai]
            pr = tp[ti] / (fp[ti] + tp[ti] + np.spacing(1))
            recall[ti, ai] = rc[-1] if len(rc) else 0
            env = np.maximum.accumulate(pr[::-1])[::-1]          # the precision envelope
            inds = np.searchsorted(rc, REC_THRS, side="left")
            q = np.zeros(R)
            q[inds < len(env)] = env[inds[inds < len(env)]]
            precision[ti, :, ai] = q

    def mean(x):
        x = x[x > -1]
        return float(x.mean()) if x.size else -1.0
    stats = np.array([mean(precision[:, :, 0]), mean(precision[0, :, 0]), mean(precision[5, :, 0]), mean(precision[:, :, 1]),
                      mean(precision[:, :, 2]), mean(recall[:, 0]), mean(recall[0:1, 0]), mean(recall[5:6, 0]), mean(recall[:, 1]),
                      mean(recall[:, 2])])
    return dict(precision=precision, recall=recall, stats=stats, margin=margin)


# ------------------------------------------------------------------------------------------------ hand cases (test_evaluate_cpu.py's)
def person(cx, cy, img, ann_id, area=80.0 * 80.0, vis=2, crowd=0, nk=17):
    k = np.zeros((17, 3))
    k[:, 0] = cx + 20 * np.cos(np.arange(17))
    k[:, 1] = cy + 30 * np.sin(np.arange(17))
    k[:, 2] = vis
    return dict(id=ann_id, image_id=img, category_id=1, keypoints=k.reshape(-1).tolist(), num_keypoints=nk, area=area,
                bbox=[cx - 40, cy - 40, 80, 80], iscrowd=crowd)


def det(gt, score, shift=0.0):
    k = np.array(gt["keypoints"]).reshape(17, 3).copy()
    k[:, 0] += shift
    k[:, 2] = 0.9
    return dict(image_id=gt["image_id"], category_id=1, keypoints=k.reshape(-1).tolist(), score=score)


def straddle_shift(gt):
    """A shift whose OKS lies between 0.5 and 0.75."""
    var = (COCO_SIGMAS * 2) ** 2
    return next(sh for sh in np.arange(1, 80, 0.5)
                if 0.55 < np.mean(np.exp(-(sh ** 2) / var / (gt["area"] + np.spacing(1)) / 2)) < 0.7)


def hand_cases():
    """name -> (ground truth, results): perfect, half, threshold straddle, ignored ground truth (with -1 for the empty range)."""
    gts = [person(100, 100, 1, 1), person(300, 120, 1, 2), person(150, 150, 2, 3, area=120.0 * 120.0)]
    gts2 = [person(100, 100, 1, 1), person(300, 120, 1, 2)]
    gt = person(100, 100, 1, 1)
    gts3 = [person(100, 100, 1, 1), person(300, 120, 1, 2, crowd=1), person(500, 120, 1, 3, nk=0)]
    return {"perfect": (gts, [det(g, 0.9 - 0.1 * i) for i, g in enumerate(gts)]),
            "half": (gts2, [det(gts2[0], 0.9), det(gts2[1], 0.8, shift=500.0)]),
            "straddle": ([gt], [det(gt, 0.9, shift=straddle_shift(gt))]),
            "ignored": (gts3, [det(gts3[0], 0.9), det(gts3[1], 0.95), det(gts3[2], 0.97)])}


# ------------------------------------------------------------------------------------------------ seeded sets
def _pose(rng, cx, cy, size):
    k = np.zeros((17, 3))
    k[:, 0] = cx + size * rng.uniform(-0.5, 0.5, 17)
    k[:, 1] = cy + size * rng.uniform(-0.5, 0.5, 17)
    return k


def ap_set(seed=11):
    """64 images (ids 1 .. 64, shuffled lists): 0 .. 8 ground truths each, one image with 65 and one with 128; crowds, persons with
    num_keypoints == 0 (no labelled joint: the box-distance branch), partly labelled persons, areas exactly 32^2 and 96^2, images
    with detections only and with ground truth only, one with 30 detections, zero scores tied across images, results with and
    without "area".  Returns (annotations, results)."""
    rng = np.random.default_rng(seed)
    gts, dts, aid = [], [], 0
    for im in range(1, 65):
        ng = int(rng.integers(0, 9))
        if im == 7:
            ng = 65
        if im == 23:
            ng = 128
        if im in (5, 40):
            ng = 0               # detections only
        mine = []
        for _ in range(ng):
            size = float(rng.uniform(25, 220))
            cx, cy = rng.uniform(0, 640), rng.uniform(0, 480)
            k = _pose(rng, cx, cy, size)
            kind = rng.random()
            if kind < 0.12:      # no labelled joint
                k[:] = 0.0
            elif kind < 0.5:     # partly labelled
                k[:, 2] = rng.integers(0, 3, 17)
                k[k[:, 2] == 0, :2] = 0.0
            else:
                k[:, 2] = 2
            area = float(size * size * rng.uniform(0.4, 0.9))
            r = rng.random()
            area = 32.0 ** 2 if r < 0.08 else (96.0 ** 2 if r < 0.16 else area)
            aid += 1
            g = dict(id=aid, image_id=im, category_id=1, keypoints=k.reshape(-1).tolist(), num_keypoints=int((k[:, 2] > 0).sum()),
                     area=area, bbox=[cx - size / 2, cy - size / 2, size, size], iscrowd=int(rng.random() < 0.1))
            mine.append((g, cx, cy, size))
            gts.append(g)
        if im in (9, 50):
            mine_d = []          # ground truth only
        else:
            mine_d = [m for m in mine if rng.random() < 0.8]
        nfp = int(rng.integers(0, 4)) + (30 if im == 12 else 0)
        cand = []
        for g, cx, cy, size in mine_d:
            k = np.asarray(g["keypoints"]).reshape(17, 3).copy()
            lab = k[:, 2] > 0
            k[~lab, :2] = _pose(rng, cx, cy, size)[~lab, :2]
            k[:, :2] += rng.normal(0, size * rng.choice([0.005, 0.02, 0.05, 0.1]), (17, 2))
            k[:, 2] = rng.uniform(0.3, 1.0, 17)
            cand.append((k, g["area"]))
        for _ in range(nfp):
            size = float(rng.uniform(25, 220))
            k = _pose(rng, rng.uniform(0, 640), rng.uniform(0, 480), size)
            k[:, 2] = rng.uniform(0.3, 1.0, 17)
            cand.append((k, size * size * 0.6))
        for k, area in cand:
            score = float(rng.uniform(0.05, 1.0)) if rng.random() > 0.12 else 0.0     # zero scores: tied within and across images
            d = dict(image_id=im, category_id=1, keypoints=k.reshape(-1).tolist(), score=score)
            if rng.random() < 0.5:
                d["area"] = float(area)
            dts.append(d)
    gts = [gts[i] for i in _interleave(rng, [g["image_id"] for g in gts])]
    dts = [dts[i] for i in _interleave(rng, [d["image_id"] for d in dts])]
    return gts, dts


def _interleave(rng, ids):
    """An order that interleaves the rows of different images and keeps the order within each."""
    ids = np.asarray(ids)
    key = rng.random(len(ids))
    for im in np.unique(ids):
        key[ids == im] = np.sort(key[ids == im])
    return np.argsort(key, kind="mergesort")


NMS_SIZES = (1, 2, 16, 17, 64, 65, 300, 1024)


def nms_set(seed=3, dtype=np.float64):
    """A ragged set with images of NMS_SIZES persons, their rows interleaved: clusters of near-duplicates around a few poses, exact
    duplicates (OKS exactly 1, another box score), and -- in the images of at most 16 persons only -- persons without a confident
    joint (score exactly 0, several tied).  Returns (preds [P, 17, 3] dtype, boxes [P, 6] float64, image ids [P])."""
    rng = np.random.default_rng(seed)
    preds, boxes, ids = [], [], []
    for im, n in enumerate(NMS_SIZES):
        ncl = max(1, n // 12)
        centres = [(rng.uniform(0, 640), rng.uniform(0, 480), float(rng.uniform(60, 200))) for _ in range(ncl)]
        bases = [_pose(rng, cx, cy, s) for cx, cy, s in centres]
        rows = []
        for p in range(n):
            c = int(rng.integers(0, ncl))
            s = centres[c][2]
            if rows and rng.random() < 0.08:
                k = rows[int(rng.integers(0, len(rows)))][0].copy()      # an exact duplicate
            else:
                k = bases[c].copy()
                k[:, :2] += rng.normal(0, s * rng.choice([0.002, 0.01, 0.03, 0.2]), (17, 2))
                k[:, 2] = rng.uniform(0.05, 1.0, 17)
                if n <= 16 and n > 1 and rng.random() < 0.4:
                    k[:, 2] = rng.uniform(0.0, 0.19, 17)                  # nothing above the visibility threshold
            area = s * s * float(rng.uniform(0.5, 1.0))
            rows.append((k, [centres[c][0], centres[c][1], s / 200, s / 200, area, float(rng.uniform(0.1, 1.0))]))
        if n == 16:   # three zero scores for certain
            for p in (3, 8, 9):
                rows[p][0][:, 2] = rng.uniform(0.0, 0.19, 17)
        preds += [r[0] for r in rows]
        boxes += [r[1] for r in rows]
        ids += [100 + im] * n
    order = _interleave(rng, ids)
    preds, boxes, ids = np.asarray(preds)[order], np.asarray(boxes, np.float64)[order], np.asarray(ids)[order]
    return preds.astype(dtype), boxes, ids
