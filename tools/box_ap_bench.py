#!/usr/bin/env python3
"""Box AP benchmark (GPU only): `python tools/box_ap_bench.py OUTDIR [--images N]` writes OUTDIR/box_ap_bench.json.

A synthetic set of COCO val2017's size: 5 000 images, 100 detections and about 7 ground truths each, once with 1 category and
once with 80.  Per case:
  device_s     CocoEvaluator.accumulate() + summarize() after the last update(), the device synchronised before and after;
               median of 3.  That is everything between the last forward pass and the 12 numbers: table building, the argument
               checks of the two ops, stlpose::box_ap_match, the two sorts, stlpose::box_ap_accumulate and the host means.
  match_s / order_s / accumulate_s   the three device steps alone (device events, median of 3).
  yardstick_host_s   tests/box_ap_ref.box_ap, the fp64 numpy restatement, on the same tables (wall clock, once).
  forward_s    the D0 bf16 forward time over the same number of images, from profiles/detector_bench.json (batch 32).
No target is set.  The script fails only when the device result differs from the yardstick's: precision and recall are compared
with np.array_equal.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic(images: int, cats: int, seed: int):
    """Ground-truth annotations and per-image predictions (xyxy float32, integer coordinates: every conversion is exact)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gts, preds = [], {}
    for i in range(images):
        ng = int(rng.integers(3, 12))
        xy = rng.integers(0, 500, (ng, 2))
        wh = rng.integers(8, 200, (ng, 2))
        gc = rng.integers(1, cats + 1, ng)
        for (x, y), (w, h), c in zip(xy.tolist(), wh.tolist(), gc.tolist()):
            gts.append(dict(image_id=i, category_id=c, bbox=[float(x), float(y), float(w), float(h)], area=float(w * h),
                            iscrowd=int(rng.random() < .05)))
        src = rng.integers(0, ng, 100)
        jit = rng.integers(-12, 13, (100, 4))
        jit[rng.random(100) < .3] = 0
        x1y1 = xy[src] + jit[:, :2]
        x2y2 = x1y1 + np.maximum(wh[src] + jit[:, 2:], 1)
        lab = np.where(rng.random(100) < .8, gc[src], rng.integers(1, cats + 1, 100))
        preds[i] = dict(boxes=torch.from_numpy(np.concatenate([x1y1, x2y2], 1).astype(np.float32)),
                        labels=torch.from_numpy(lab.astype(np.int64)),
                        scores=torch.from_numpy((rng.integers(1, 1 << 16, 100) / np.float32(1 << 16)).astype(np.float32)))
    return gts, preds


def results_of(preds):
    out = []
    for img, p in preds.items():
        b = p["boxes"]
        xywh = torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], 1).double().tolist()
        for bb, l, s in zip(xywh, p["labels"].tolist(), p["scores"].tolist()):
            out.append(dict(image_id=img, category_id=l, bbox=bb, score=s))
    return out


def median3(fn):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


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
        raise SystemExit("box_ap_bench: no GPU")
    import box_ap_ref as R
    from stlpose_amd import CocoEvaluator, detection_eval as DE
    os.makedirs(outdir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "images": images, "detections_per_image": 100, "cases": {}}
    try:
        rows = json.load(open(os.path.join(ROOT, "profiles", "detector_bench.json")))["rows"]
        ips = max(r["native_imgs_per_s"] for r in rows if r["model"] == "d0" and r["dtype"] == "bf16")
        res["forward_s"] = images / ips
        res["forward_source"] = f"profiles/detector_bench.json: D0 bf16, {ips:.0f} images/s"
    except (OSError, KeyError, ValueError):
        res["forward_s"] = None
    ok = True
    for cats in (1, 80):
        gts, preds = synthetic(images, cats, cats)
        ds = dict(annotations=gts, categories=[dict(id=c) for c in range(1, cats + 1)])
        ev = CocoEvaluator(ds)
        items = list(preds.items())
        for i in range(0, len(items), 32):
            ev.update(dict(items[i:i + 32]))
        state = {}

        def run():
            ev._tables = None
            ev.synchronize_between_processes()
            ev.accumulate()
            with contextlib.redirect_stdout(io.StringIO()):
                state["stats"] = ev.summarize()["bbox"]
        run()   # warm-up: library load, allocator
        device_s = median3(run)
        got = ev.coco_eval["bbox"]
        # the three device steps alone
        uniq, boxes, scores, labels, off = ev._tables
        gt = ev.gt.select(uniq)[:5]
        cat_t = torch.arange(1, cats + 1)
        thr, rng_ = [float(t) for t in DE.IOU_THRS], [float(v) for r in DE.AREA_RANGES for v in r]
        match_s, (score, cat, rank, matched, ignored, npig) = events3(
            lambda: torch.ops.stlpose.box_ap_match(boxes, scores, labels, off, *gt, cat_t, thr, rng_))

        def order_fn():
            by_score = torch.sort(score, descending=True, stable=True).indices
            order = by_score[torch.sort(cat[by_score], stable=True).indices]
            return order, torch.cumsum(torch.bincount((cat + 1).long(), minlength=cats + 1), 0)
        order_s, (order, cat_offsets) = events3(order_fn)
        np_all = npig.sum(0, dtype=torch.int64)
        acc_s, _ = events3(lambda: torch.ops.stlpose.box_ap_accumulate(matched, ignored, rank, order, cat_offsets, np_all, 10,
                                                                       [1, 10, 100], [float(r) for r in DE.REC_THRS]))
        t0 = time.perf_counter()
        want = R.box_ap(gts, results_of(preds), img_ids=list(preds), cat_ids=list(range(1, cats + 1)))
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(got.precision, want["precision"]) and np.array_equal(got.recall, want["recall"])
                    and np.array_equal(state["stats"], want["stats"]))
        ok = ok and same
        res["cases"][f"categories_{cats}"] = {
            "categories": cats, "ground_truths": len(gts), "detections": images * 100, "device_s": device_s, "match_s": match_s,
            "order_s": order_s, "accumulate_s": acc_s, "yardstick_host_s": host_s, "speedup_vs_yardstick": host_s / device_s,
            "share_of_forward": device_s / res["forward_s"] if res["forward_s"] else None, "equals_yardstick": same,
            "stats": [float(v) for v in state["stats"]]}
        print(json.dumps(res["cases"][f"categories_{cats}"]), flush=True)
    with open(os.path.join(outdir, "box_ap_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not ok:
        raise SystemExit("box_ap_bench: the device result differs from the yardstick")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="box AP benchmark")
    ap.add_argument("outdir")
    ap.add_argument("--images", type=int, default=5000)
    a = ap.parse_args()
    main(a.outdir, a.images)
