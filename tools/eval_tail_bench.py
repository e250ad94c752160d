#!/usr/bin/env python3
"""Evaluation-tail benchmark (GPU only): `python tools/eval_tail_bench.py OUTDIR [--batches N]` writes OUTDIR/eval_tail_bench.json.

The workload of bench.py's extra_eval_path: HRNet-W32, mixed, 384 x 288, batches of 32 (one cached synthetic batch), 10 batches,
4 persons per image, flip test.  Evaluator(tail="host") and Evaluator(tail="device") run the same epoch alternately in one process
(host, device, host, device, ...), the device synchronised before and after each epoch; the figure of a tail is the median of its 3
epochs, in ms per batch, host post-processing (rescoring, OKS-NMS) included.
  tail_launches_ms   device time of the two launches EvalTables.add lists for one batch (stlpose::eval_tail = stl_eval_tail +
                     stl_sum_partials) on heat maps of the run's size, from device events; median of 5.
  affine_ms          the epoch's one stl_eval_affine launch, likewise.
  device_tail_device_scoring_ms_per_batch   the device tail with scoring="device" (rescoring and OKS-NMS on the device as well, fed
                     the device tensor), 3 epochs after the alternating ones, median; not part of the acceptance.
  loadavg            the host's 1-minute load average before and after the run, and its CPU count: the host tail's figure moves
                     with it.
The script fails when the two tails' results differ, or when the device tail's median is above the host tail's.
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


def events(fn, n=5):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main(outdir, batches, batch=32, H=384, W=288, persons_per_image=4):
    if not torch.cuda.is_available():
        raise SystemExit("eval_tail_bench: no GPU")
    from bench import synth_batch
    from stlpose_amd import EvalTables, PoseHighResolutionNet
    from stlpose_amd.evaluate import Evaluator
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda:0")
    load0 = os.getloadavg()[0]
    torch.manual_seed(0)
    model = PoseHighResolutionNet("w32", "mixed").to(dev).eval()
    img, tgt, tw = synth_batch(batch, H, W, 0, dev, sigma=3.0)

    def loader(n):
        rng = np.random.Generator(np.random.PCG64(5))
        for bi in range(n):
            ids = (bi * batch + np.arange(batch)) // persons_per_image
            yield img, tgt, tw, dict(center=rng.uniform(100, 400, (batch, 2)), scale=rng.uniform(0.8, 2.0, (batch, 2)),
                                     score=rng.uniform(0.3, 1.0, batch), image_id=ids)
    evs = {t: Evaluator(model, device=dev, flip=True, tail=t) for t in ("host", "device")}
    out = {t: evs[t].evaluate_model(loader(2)) for t in evs}   # warm-up: plan, lazy kernel attributes, allocator
    times = {t: [] for t in evs}
    for _ in range(3):
        for t in evs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[t] = evs[t].evaluate_model(loader(batches))
            torch.cuda.synchronize()
            times[t].append((time.perf_counter() - t0) / batches * 1e3)
    both = Evaluator(model, device=dev, flip=True, tail="device", scoring="device")
    both.evaluate_model(loader(2))
    times_both = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out_both = both.evaluate_model(loader(batches))
        torch.cuda.synchronize()
        times_both.append((time.perf_counter() - t0) / batches * 1e3)
    same = out["host"]["results"] == out["device"]["results"] and out["host"]["accuracy"] == out["device"]["accuracy"] \
        and abs(out["host"]["loss"] - out["device"]["loss"]) <= 2.0 ** -23 * abs(out["host"]["loss"])

    # the new launches alone, on the model's own heat maps
    with torch.no_grad():
        o, of = model(img.float().to(dev)), model(img.float().to(dev).flip(3))
    t_dev, tw_dev = tgt.float().to(dev), tw.float().to(dev)
    tables = EvalTables(dev, joints=o.shape[1])
    tables.add(o, of, t_dev, tw_dev)
    tail_ms = events(lambda: tables.add(o, of, t_dev, tw_dev))
    n = tables.rows
    c, s = torch.rand(n, 2, device=dev) * 300 + 100, torch.rand(n, 2, device=dev) + 0.8
    affine_ms = events(lambda: torch.ops.stlpose.eval_affine(tables._tables[2], tables._tables[3], c, s, o.shape[2], o.shape[3]))
    med = {t: float(np.median(times[t])) for t in times}
    res = {"device": torch.cuda.get_device_name(0), "workload": f"HRNet-W32 mixed {H}x{W} bs={batch}, {batches} batches, flip test, "
           f"{persons_per_image} persons per image", "host_tail_ms_per_batch": med["host"], "device_tail_ms_per_batch": med["device"],
           "host_tail_runs_ms_per_batch": times["host"], "device_tail_runs_ms_per_batch": times["device"],
           "host_tail_images_per_s": batch / med["host"] * 1e3, "device_tail_images_per_s": batch / med["device"] * 1e3,
           "device_tail_device_scoring_ms_per_batch": float(np.median(times_both)),
           "tail_launches_ms": tail_ms, "affine_ms": affine_ms, "affine_rows": n, "equal_results": bool(same),
           "equal_results_device_scoring": out_both["results"] == out["host"]["results"],
           "results": len(out["device"]["results"]),
           "loadavg": {"before": load0, "after": os.getloadavg()[0], "cpus": os.cpu_count()}}
    with open(os.path.join(outdir, "eval_tail_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not same:
        raise SystemExit("eval_tail_bench: the device tail's results differ from the host tail's")
    if not med["device"] <= med["host"]:
        raise SystemExit("eval_tail_bench: the device tail is slower than the host tail")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="evaluation tail benchmark")
    ap.add_argument("outdir")
    ap.add_argument("--batches", type=int, default=10)
    a = ap.parse_args()
    main(a.outdir, a.batches)
