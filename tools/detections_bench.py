#!/usr/bin/env python3
"""The detector's tail on one MI355X: from the head outputs to detections, on the host path (decode launch, per image a sort, three
NMS launches and the copies: EfficientDetBackbone.detect) and on the device path (one stlpose::det_postprocess launch, then
either Detections.to_list -- one copy -- or DetectionStore.append -- one launch, no copy).  D0, bf16, batches 8 and 32,
threshold 0.5, seeded random weights; the classifier's last bias is shifted so that an image carries about TARGET candidates
(the shift and the candidate counts found are recorded).  Host and device alternate in one process; every figure is the median
of ROUNDS wall-clock times with the device synchronised before and after.  The two lists must be equal, and the device tail must
be faster than the host tail at batch 32, or the script fails.
Usage: python tools/detections_bench.py OUTDIR -> OUTDIR/detections_bench.json (commit it as profiles/detections_bench.json)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import efficientdet as E  # noqa: E402
from stlpose_amd.detections import DetectionStore  # noqa: E402

SEED, TARGET, THR, IOU, ROUNDS, MODE = 0, 150, 0.5, 0.5, 3, "bf16"
DEV = "cuda"


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def same(a, b):
    return len(a) == len(b) and all(x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "labels", "scores"))


def main(outdir):
    torch.manual_seed(SEED)
    m = E.setup_detector("efficientdet", "d0", compute_dtype=MODE).to(DEV).eval()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(SEED + 1)
    images = {b: torch.rand(b, 3, 384, 512, generator=gen).to(DEV) for b in (8, 32)}
    # the shift that leaves TARGET candidates per image at THR: the TARGET * B-th largest best-class logit moves to 0
    _, _, cls, _ = m(images[32], postprocess=False)
    best = cls.amax(2).double().clamp(1e-12, 1 - 1e-12)
    logit = torch.log(best / (1 - best)).flatten()
    shift = -float(torch.topk(logit, TARGET * 32).values[-1])
    with torch.no_grad():
        m.classifier.header.pointwise_conv.conv.bias += shift
    out = dict(model="d0", compute_dtype=MODE, threshold=THR, iou_threshold=IOU, weight_seed=SEED, class_bias_shift=shift,
               rounds=ROUNDS, device=torch.cuda.get_device_name(0), batches={})
    for b, x in images.items():
        srcs = m._float_sources(x, dev)
        store = DetectionStore(1 << 20, dev)
        ids = list(range(b))
        state = {}

        def heads():
            state["p"], state["metas"] = m.run_raw(srcs, 1, dev)

        def host_tail():
            state["host"] = m.detect(state["p"], state["metas"], THR, IOU)

        def device_list():
            state["device"] = m.detect(state["p"], state["metas"], THR, IOU, output="device").to_list()

        def device_store():
            store.append(ids, m.detect(state["p"], state["metas"], THR, IOU, output="device"))

        legs = {"host_tail_ms": host_tail, "device_tail_to_list_ms": device_list, "device_tail_to_store_ms": device_store,
                "forward_ms": heads,
                "host_forward_and_tail_ms": lambda: m(x, threshold=THR, iou_threshold=IOU),
                "device_forward_and_list_ms": lambda: m(x, threshold=THR, iou_threshold=IOU, output="device").to_list(),
                "device_forward_and_store_ms": lambda: store.append(ids, m(x, threshold=THR, iou_threshold=IOU, output="device"))}
        heads()
        for fn in legs.values():   # warm-up: plans, allocator, first launches
            fn()
        times = {k: [] for k in legs}
        for _ in range(ROUNDS):    # the legs alternate within a round
            heads()
            for k, fn in legs.items():
                times[k].append(wall_ms(fn))
        if not same(state["host"], state["device"]):
            raise SystemExit(f"batch {b}: the device list differs from the host list")
        rec = {k: statistics.median(v) for k, v in times.items()}
        rec["all_times_ms"] = times
        counts = [len(d["scores"]) for d in state["host"]]
        cand = (state["p"].cls.amax(2) > THR).sum(1).tolist()
        rec.update(candidates_per_image=dict(min=min(cand), median=statistics.median(cand), max=max(cand)),
                   detections_per_image=dict(min=min(counts), median=statistics.median(counts), max=max(counts)),
                   host_over_device_tail_to_list=rec["host_tail_ms"] / rec["device_tail_to_list_ms"],
                   host_over_device_tail_to_store=rec["host_tail_ms"] / rec["device_tail_to_store_ms"],
                   host_launches=1 + 4 * sum(c > 0 for c in cand), device_launches_to_list=2, device_launches_to_store=2)
        out["batches"][str(b)] = rec
        print(json.dumps({k: v for k, v in rec.items() if k != "all_times_ms"}), flush=True)
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "detections_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    r = out["batches"]["32"]
    if not r["device_tail_to_list_ms"] < r["host_tail_ms"]:
        raise SystemExit(f"batch 32: device tail {r['device_tail_to_list_ms']:.3f} ms is not faster than the host tail {r['host_tail_ms']:.3f} ms")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles"))
