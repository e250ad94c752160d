#!/usr/bin/env python3
"""Top-down extraction benchmark (GPU only): `python tools/topdown_bench.py OUTDIR` writes OUTDIR/topdown_bench.json.

Legs:
  decode     512 persons x 17 maps, 64 x 48 -> 256 x 192: the fused stlpose::heatmap_resize_argmax, against F.interpolate +
             stlpose::heatmap_argmax on the device, and the reference's path (F.interpolate on the device, .cpu(), np.argmax /
             np.amax on the host).  Bytes model: the fused kernel reads the maps once (209 KB per person) and writes 17 x 4 values;
             the unfused path also writes the 256 x 192 maps and reads them back (2 x 3.3 MB per person).
  nms        16 images x 1000 boxes, IoU 0.5: stlpose::box_select (one launch) against the numpy restatement tests/topdown_ref.nms.
  extractor  PoseExtractor on W32 256 x 192: persons per second (192 persons in 16 images, chunks of 32), flip off / on, in the
             mixed and fp32 compute modes, synthetic weights.
Times are device events around `reps` calls after a warm-up (host legs: wall clock).
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BW = 8.0e12


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def wall(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main(outdir):
    if not torch.cuda.is_available():
        raise SystemExit("topdown_bench: no GPU")
    import stlpose_amd  # noqa: F401
    from oracle import hrnet_ref
    from stlpose_amd import PoseExtractor, PoseHighResolutionNet
    import topdown_ref as R
    os.makedirs(outdir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "legs": {}}
    L = res["legs"]

    # ---- decode
    B, J, h, w, ho, wo = 512, 17, 64, 48, 256, 192
    gen = torch.Generator(device="cuda").manual_seed(0)
    hm = torch.rand(B, J, h, w, device="cuda", generator=gen)
    fused = timed(lambda: torch.ops.stlpose.heatmap_resize_argmax(hm, ho, wo), reps=20)
    unfused = timed(lambda: torch.ops.stlpose.heatmap_argmax(F.interpolate(hm, (ho, wo), mode="bilinear", align_corners=True)), reps=10)

    def host():
        up = F.interpolate(hm, (ho, wo), mode="bilinear", align_corners=True).cpu().numpy().reshape(B, J, -1)
        return np.argmax(up, 2), np.amax(up, 2)
    ref = wall(host, reps=2)
    src_b, up_b = B * J * h * w * 4, B * J * ho * wo * 4
    L["decode"] = {"persons": B, "maps": f"{J} x {h} x {w} -> {ho} x {wo}",
                   "fused_s": fused, "unfused_device_s": unfused, "reference_host_s": ref,
                   "fused_bytes": src_b, "unfused_bytes": src_b + 2 * up_b,
                   "fused_gbytes_per_s": src_b / fused / 1e9, "unfused_gbytes_per_s": (src_b + 2 * up_b) / unfused / 1e9,
                   "speedup_vs_unfused_device": unfused / fused, "speedup_vs_reference": ref / fused,
                   "fused_share_of_hbm_peak": src_b / PEAK_BW / fused}

    # ---- nms
    rng = np.random.default_rng(1)
    ni, nb = 16, 1000
    xy = rng.uniform(0, 1000, (ni * nb, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(10, 200, (ni * nb, 2))], 1).astype(np.float32)
    scores = rng.uniform(0, 1, ni * nb).astype(np.float32)
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    off = torch.arange(0, ni * nb + 1, nb, dtype=torch.int64)
    dev = timed(lambda: torch.ops.stlpose.box_select(b, s, None, off, 1, None, 0.5), reps=20)
    t0 = time.perf_counter()
    kept = [len(R.nms(boxes[i * nb:(i + 1) * nb], scores[i * nb:(i + 1) * nb], 0.5)) for i in range(ni)]
    host_s = time.perf_counter() - t0
    _, count = torch.ops.stlpose.box_select(b, s, None, off, 1, None, 0.5)
    assert count.cpu().tolist() == kept
    L["nms"] = {"images": ni, "boxes_per_image": nb, "iou_thr": 0.5, "kept_mean": float(np.mean(kept)), "box_select_s": dev,
                "numpy_restatement_s": host_s, "speedup": host_s / dev}

    # ---- extractor
    images = [torch.from_numpy(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)) for _ in range(16)]
    pboxes = []
    for _ in images:
        xy = rng.uniform(0, 400, (12, 2))
        pboxes.append(np.concatenate([xy, xy + rng.uniform(60, 220, (12, 2))], 1).astype(np.float32))
    persons = sum(len(x) for x in pboxes)
    L["extractor"] = {"persons": persons, "images": len(images), "batch": 32, "arch": "w32", "input": "256 x 192"}
    for mode in ("mixed", "fp32"):
        model = PoseHighResolutionNet("w32", mode)
        sd = {k: torch.from_numpy(hrnet_ref.synth_tensor(k, tuple(v.shape))) for k, v in model.state_dict().items()}
        model.load_state_dict(sd, strict=True)
        model = model.cuda().eval()
        for flip in (False, True):
            ex = PoseExtractor(model, flip=flip, batch=32)
            sec = wall(lambda: ex(images, pboxes), reps=3)
            L["extractor"][f"{mode}_flip{int(flip)}"] = {"seconds": sec, "persons_per_s": persons / sec}
        del model
        torch.cuda.empty_cache()
    with open(os.path.join(outdir, "topdown_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: topdown_bench.py OUTDIR")
    main(sys.argv[1])
