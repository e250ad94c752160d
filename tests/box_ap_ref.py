"""fp64 numpy restatement of the published COCOeval for iouType "bbox" (pycocotools: maskApi.bbIou, COCOeval.evaluateImg,
accumulate, summarize), the yardstick of stlpose_amd.detection_eval and csrc/box_ap.hip.  Plain loops, nothing imported from the
package.  pycocotools itself is not installed: tests/test_box_ap_cpu.py pins this file with hand-computed cases.

The per-image step is kept apart from the accumulation (``evaluate_images`` -> ``accumulate``) so that a test can feed the
accumulation synthetic matches."""
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RANGES = [(0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2)]   # all, small, medium, large
MAX_DETS = (1, 10, 100)


def bb_iou(d, g, crowd):
    """maskApi.bbIou for one pair of (x, y, w, h) boxes."""
    ga, da = g[2] * g[3], d[2] * d[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def evaluate_image(gts, dts, area_ranges=AREA_RANGES, iou_thrs=IOU_THRS, max_det=MAX_DETS[-1]):
    """evaluateImg for one (image, category) and every area range.  gts: dicts with bbox, area, iscrowd; dts: dicts with bbox, score.
    Returns None when both are empty, else per area range a dict(scores [D], matched [T, D] bool, ignored [T, D] bool, npig)."""
    if not gts and not dts:
        return None
    order = np.argsort([-float(d["score"]) for d in dts], kind="mergesort")[:max_det]
    dts = [dts[i] for i in order]
    dbox = [[float(v) for v in d["bbox"]] for d in dts]
    out = []
    for lo, hi in area_ranges:
        gig = [bool(g.get("iscrowd", 0)) or g["area"] < lo or g["area"] > hi for g in gts]
        gorder = np.argsort(np.asarray(gig, bool), kind="mergesort") if gts else []
        gs = [gts[i] for i in gorder]
        gig = [gig[i] for i in gorder]
        crowd = [bool(g.get("iscrowd", 0)) for g in gs]
        gbox = [[float(v) for v in g["bbox"]] for g in gs]
        iou = [[bb_iou(d, g, c) for g, c in zip(gbox, crowd)] for d in dbox]
        T, D, G = len(iou_thrs), len(dts), len(gs)
        matched, ignored = np.zeros((T, D), bool), np.zeros((T, D), bool)
        for ti, t in enumerate(iou_thrs):
            gtm = [False] * G
            for di in range(D):
                best, m = min(t, 1 - 1e-10), -1
                for gi in range(G):
                    if gtm[gi] and not crowd[gi]:       # already matched, and not a crowd
                        continue
                    if m > -1 and not gig[m] and gig[gi]:   # holds a regular ground truth: stop at the ignored ones
                        break
                    if iou[di][gi] < best:
                        continue
                    best, m = iou[di][gi], gi
                if m == -1:
                    continue
                matched[ti, di], ignored[ti, di], gtm[m] = True, gig[m], True
        for di, b in enumerate(dbox):   # an unmatched detection outside the area range is ignored
            area = b[2] * b[3]
            if area < lo or area > hi:
                ignored[:, di] |= ~matched[:, di]
        out.append(dict(scores=np.array([float(d["score"]) for d in dts]), matched=matched, ignored=ignored,
                        npig=sum(1 for v in gig if not v)))
    return out


def accumulate(per_image, max_dets=MAX_DETS, rec_thrs=REC_THRS, num_thrs=len(IOU_THRS)):
    """COCOeval.accumulate.  per_image[k][i]: evaluate_image's result for category k and the i-th image (images ascending), or None.
    Returns precision [T, R, K, A, M] and recall [T, K, A, M], -1 where there is nothing to find."""
    K, T, R, M = len(per_image), num_thrs, len(rec_thrs), len(max_dets)
    A = max([len(e) for row in per_image for e in row if e is not None], default=len(AREA_RANGES))
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            E = [e[a] for e in per_image[k] if e is not None]
            if not E:
                continue
            npig = sum(e["npig"] for e in E)
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                scores = np.concatenate([e["scores"][:md] for e in E])
                order = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["matched"][:, :md] for e in E], axis=1)[:, order]
                dig = np.concatenate([e["ignored"][:, :md] for e in E], axis=1)[:, order]
                tps = np.cumsum(dtm & ~dig, axis=1).astype(float)
                fps = np.cumsum(~dtm & ~dig, axis=1).astype(float)
                for ti in range(T):
                    tp, fp = tps[ti], fps[ti]
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    recall[ti, k, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):       # the precision envelope
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[ti, :, k, a, mi] = q
    return precision, recall


def summarize(precision, recall, iou_thrs=IOU_THRS):
    """COCOeval.summarize for "bbox": AP, AP50, AP75, AP(S), AP(M), AP(L) at the last maxDets, AR at the three maxDets, AR(S), AR(M),
    AR(L) at the last; each the mean of the entries > -1, or -1."""
    def mean(x):
        x = x[x > -1]
        return float(np.mean(x)) if x.size else -1.0
    t50, t75 = int(np.where(iou_thrs == .5)[0][0]), int(np.where(iou_thrs == .75)[0][0])
    return np.array([mean(precision[:, :, :, 0, 2]), mean(precision[t50, :, :, 0, 2]), mean(precision[t75, :, :, 0, 2]),
                     mean(precision[:, :, :, 1, 2]), mean(precision[:, :, :, 2, 2]), mean(precision[:, :, :, 3, 2]),
                     mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
                     mean(recall[:, :, 1, 2]), mean(recall[:, :, 2, 2]), mean(recall[:, :, 3, 2])])


def evaluate_images(gt_annotations, results, img_ids=None, cat_ids=None, max_dets=MAX_DETS):
    """per_image[k][i] for the images (ascending ids) and categories (ascending ids) evaluated; also returns both id lists."""
    gt_by, dt_by = defaultdict(list), defaultdict(list)
    for g in gt_annotations:
        gt_by[g["image_id"], g["category_id"]].append(g)
    for d in results:
        dt_by[d["image_id"], d["category_id"]].append(d)
    if img_ids is None:
        img_ids = {g["image_id"] for g in gt_annotations} | {d["image_id"] for d in results}
    if cat_ids is None:
        cat_ids = {g["category_id"] for g in gt_annotations} | {d["category_id"] for d in results}
    img_ids, cat_ids = sorted(set(img_ids)), sorted(set(cat_ids))
    per_image = [[evaluate_image(gt_by.get((i, c), []), dt_by.get((i, c), []), max_det=max_dets[-1]) for i in img_ids] for c in cat_ids]
    return per_image, img_ids, cat_ids


def box_ap(gt_annotations, results, img_ids=None, max_dets=MAX_DETS, cat_ids=None):
    """The whole evaluation: dict(stats [12], precision [T, R, K, A, M], recall [T, K, A, M])."""
    per_image, _, _ = evaluate_images(gt_annotations, results, img_ids, cat_ids, max_dets)
    precision, recall = accumulate(per_image, max_dets)
    return dict(stats=summarize(precision, recall), precision=precision, recall=recall)
