#!/usr/bin/env python3
"""Pose scoring benchmark (GPU only): `python tools/keypoint_eval_bench.py OUTDIR [--images N]` writes OUTDIR/keypoint_eval_bench.json.

A synthetic set of COCO val2017's size: 5 000 images, about 20 candidate persons (float32, several near-duplicates around each
annotated person, as overlapping detector boxes give them) and 2-3 ground truths each, seeded.
  device_s     rescore_and_nms_device + keypoint_ap (on the PoseResults, the KeypointGroundTruth built once before), the device
               synchronised before and after; median of 3.  That is everything between the last decode and the 10 numbers.
  nms_s / match_s / order_s / accumulate_s   the four device steps alone (device events, median of 3): stlpose::pose_rescore_nms,
               stlpose::oks_ap_match, the two sorts, stlpose::box_ap_accumulate.  host_s = device_s minus their sum: grouping the
               persons by image, table building, argument checks, the copies and the ten means.
  to_list_s    PoseResults.to_list(), which the Evaluator needs for its result list and preds_file (not part of device_s).
  host_path_s  evaluate.rescore_and_nms + evaluate.oks_ap on the same data (wall clock, once), and its two parts.
The script fails when the result lists or the ten numbers differ, or when the device path is not faster than the host path.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(images: int, seed: int):
    """(preds float32 [P, 17, 3], boxes [P, 6], image ids [P], annotations)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    preds, boxes, ids, gts = [], [], [], []
    for im in range(images):
        ng = int(rng.integers(2, 4))
        for _ in range(ng):
            size = float(rng.uniform(40, 220))
            cx, cy = rng.uniform(0, 640), rng.uniform(0, 480)
            k = np.zeros((17, 3))
            k[:, 0], k[:, 1] = cx + size * rng.uniform(-.5, .5, 17), cy + size * rng.uniform(-.5, .5, 17)
            k[:, 2] = rng.integers(0, 3, 17)
            gts.append(dict(id=len(gts), image_id=im, category_id=1, keypoints=k.reshape(-1).tolist(), num_keypoints=int((k[:, 2] > 0).sum()),
                            area=size * size * float(rng.uniform(.4, .9)), bbox=[cx - size / 2, cy - size / 2, size, size],
                            iscrowd=int(rng.random() < .05)))
            for _ in range(int(rng.integers(4, 9))):   # the candidates around this person
                p = k.copy()
                p[:, :2] += rng.normal(0, size * rng.choice([.003, .01, .03, .1]), (17, 2))
                p[:, 2] = rng.uniform(.05, 1., 17)
                preds.append(p), ids.append(im)
                boxes.append([cx, cy, size / 200, size / 200, size * size * float(rng.uniform(.8, 1.2)), float(rng.uniform(.1, 1.))])
        for _ in range(int(rng.integers(2, 7))):       # and some elsewhere
            size = float(rng.uniform(40, 220))
            cx, cy = rng.uniform(0, 640), rng.uniform(0, 480)
            p = np.zeros((17, 3))
            p[:, 0], p[:, 1] = cx + size * rng.uniform(-.5, .5, 17), cy + size * rng.uniform(-.5, .5, 17)
            p[:, 2] = rng.uniform(.05, .6, 17)
            preds.append(p), ids.append(im), boxes.append([cx, cy, size / 200, size / 200, size * size, float(rng.uniform(.1, 1.))])
    return np.asarray(preds, np.float32), np.asarray(boxes, np.float64), np.asarray(ids, np.int64), gts


def median3(fn):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def events3(fn):
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), out


def main(outdir, images):
    if not torch.cuda.is_available():
        raise SystemExit("keypoint_eval_bench: no GPU")
    from stlpose_amd import KeypointGroundTruth, keypoint_ap, rescore_and_nms_device
    import stlpose_amd.keypoint_eval as KE
    from stlpose_amd.evaluate import COCO_SIGMAS, oks_ap, rescore_and_nms
    os.makedirs(outdir, exist_ok=True)
    preds, boxes, ids, gts = synthetic(images, 1)
    img_ids = sorted(set(ids.tolist()))
    t0 = time.perf_counter()
    table = KeypointGroundTruth(gts)
    torch.cuda.synchronize()
    table_s = time.perf_counter() - t0

    def run():
        kept = rescore_and_nms_device(preds, boxes, ids)
        return kept, keypoint_ap(table, kept, img_ids=img_ids)
    run()   # warm-up: library load, allocator
    device_s, (kept, stats) = median3(run)
    to_list_s, results = median3(kept.to_list)

    # the device steps alone
    sig = [float(s) for s in COCO_SIGMAS]
    dp, db = torch.from_numpy(preds).cuda(), torch.from_numpy(boxes).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=images))]).astype(np.int64))   # ids ascend
    nms_s, _ = events3(lambda: torch.ops.stlpose.pose_rescore_nms(dp, db, off, 0.2, 0.9, sig))
    gt = table.select(np.asarray(img_ids))
    koff = torch.from_numpy(kept.offsets)
    thr, rng_ = [float(t) for t in KE.OKS_THRS], [float(v) for r in KE.AREA_RANGES for v in r]
    match_s, (score, cat, rank, matched, ignored, npig) = events3(
        lambda: torch.ops.stlpose.oks_ap_match(kept.keypoints, kept.scores, None, koff, *gt, thr, rng_, sig))

    def order_fn():
        by_score = torch.sort(score, descending=True, stable=True).indices
        order = by_score[torch.sort(cat[by_score], stable=True).indices]
        return order, torch.cumsum(torch.bincount((cat + 1).long(), minlength=2), 0)
    order_s, (order, cat_offsets) = events3(order_fn)
    np_all = npig.sum(0, dtype=torch.int64)
    acc_s, _ = events3(lambda: torch.ops.stlpose.box_ap_accumulate(matched, ignored, rank, order, cat_offsets, np_all, 10, [20],
                                                                   [float(r) for r in KE.REC_THRS]))
    # the host path, once
    t0 = time.perf_counter()
    want_results = rescore_and_nms(preds, boxes, ids.tolist())
    t1 = time.perf_counter()
    want_stats = oks_ap(gts, want_results, img_ids=img_ids)
    t2 = time.perf_counter()
    same_results = results == want_results
    same_stats = bool(np.array_equal(stats, want_stats))
    steps = nms_s + match_s + order_s + acc_s
    res = {"device": torch.cuda.get_device_name(0), "images": images, "candidate_persons": int(len(preds)), "ground_truths": len(gts),
           "kept_persons": len(results), "device_s": device_s, "nms_s": nms_s, "match_s": match_s, "order_s": order_s,
           "accumulate_s": acc_s, "host_s": device_s - steps,
           "shares": {k: v / device_s for k, v in (("nms", nms_s), ("match", match_s), ("order", order_s), ("accumulate", acc_s),
                                                   ("host", device_s - steps))},
           "ground_truth_table_s": table_s, "to_list_s": to_list_s,
           "host_path_s": t2 - t0, "host_rescore_and_nms_s": t1 - t0, "host_oks_ap_s": t2 - t1, "speedup": (t2 - t0) / device_s,
           "equal_results": same_results, "equal_stats": same_stats, "stats": [float(v) for v in stats]}
    with open(os.path.join(outdir, "keypoint_eval_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not (same_results and same_stats):
        raise SystemExit("keypoint_eval_bench: the device result differs from the host path's")
    if not device_s < t2 - t0:
        raise SystemExit("keypoint_eval_bench: the device path is not faster than the host path")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="pose scoring benchmark")
    ap.add_argument("outdir")
    ap.add_argument("--images", type=int, default=5000)
    a = ap.parse_args()
    main(a.outdir, a.images)
