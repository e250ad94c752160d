#!/usr/bin/env python3
"""Detector batches built on the device (stlpose_amd/det_data.py, csrc/det_batch.hip) on one MI355X: D0 at batch 8 and 32, S1 = 512,
64 resident 640 x 480 images with two boxes each, compute_dtype "fp32" and "f16".  Per (batch, mode), the legs alternating in one
process, ROUNDS times each, device synchronised, medians reported:

  loader_ms        one batch of DetBatchLoader alone (the table gathers + the one stl_det_batch launch + the metas)
  step_loader_ms   a fine-tune step fed by the loader: the batch, detection_loss(batch), backward, an SGD step over the heads
  step_host_ms     the same step fed the old way: detection_loss(imgs / 255, targets) on ONE prebuilt batch (the resized images as a
                   device tensor, the scaled boxes as host tensors), i.e. the division, the record table, stl_det_preprocess,
                   pack_targets and two uploads instead of the loader's launch
  valid_loader_ms  a validation batch: the batch + model(batch, output="device")
  valid_host_ms    model(imgs / 255, output="device") on the prebuilt batch

One gate: the loader-fed step must not be slower than the host-fed step of the same run by more than 3 % (the host-fed step contains
everything the loader-fed one does); each row records it as "loader_step_within_3pct", and the tool exits with status 1, after
writing the file, if one is false.  Usage: python tools/det_batch_bench.py OUTDIR -> OUTDIR/det_batch_bench.json (commit it as
profiles/det_batch_bench.json)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import efficientdet as E  # noqa: E402
from stlpose_amd.det_data import DetBatchLoader, DetectionDB  # noqa: E402
from stlpose_amd.pose_data import ResidentImages  # noqa: E402
from tests import detector_ref as R  # noqa: E402
from tools.detector_bench import timed  # noqa: E402

ROUNDS = 3
MODES = ("fp32", "f16")
S1, N_IMAGES, H, W = 512, 64, 480, 640
BOXES = np.array([[60.0, 40.0, 180.0, 160.0], [230.0, 110.0, 330.0, 290.0]], np.float32)
SLACK = 1.03


def table() -> DetectionDB:
    n = N_IMAGES
    return DetectionDB(image_id=np.arange(n, dtype=np.int64), file_name=[f"{k}.jpg" for k in range(n)],
                       original_name=[f"{k}.jpg" for k in range(n)], height=np.full(n, H, np.int32), width=np.full(n, W, np.int32),
                       perceptual_loss=np.zeros(n), box_start=2 * np.arange(n, dtype=np.int64), box_count=np.full(n, 2, np.int32),
                       boxes=np.tile(BOXES, (n, 1)), labels=np.ones(2 * n, np.int64), area=np.ones(2 * n))


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    db = table()
    store = ResidentImages.from_arrays([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N_IMAGES)], dev)
    models = {}
    for mode in MODES:
        m = E.setup_detector("efficientdet", "d0", compute_dtype=mode)
        sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        # the training tests' classifier header: scores inside the loss's clamp
        sd["classifier.header.pointwise_conv.conv.weight"] = sd["classifier.header.pointwise_conv.conv.weight"] * 0.1
        sd["classifier.header.pointwise_conv.conv.bias"] = torch.full_like(sd["classifier.header.pointwise_conv.conv.bias"], -2.0)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        heads = [p for k, p in m.named_parameters() if k.startswith(("regressor.", "classifier."))]
        models[mode] = (m, torch.optim.SGD(heads, lr=1e-6))
    rows = []
    for B in (8, 32):
        loader = DetBatchLoader(db, store, None, B, False, image_size=S1, stage1=True, device=dev)
        first, _ = loader[0]
        imgs = first.stage1.permute(0, 3, 1, 2).float().contiguous()          # the prebuilt host-style batch, values 0 .. 255
        scaled = db.scaled_boxes(S1)
        targets = [{"boxes": torch.from_numpy(scaled[2 * k:2 * k + 2].copy()), "labels": torch.ones(2, dtype=torch.long)} for k in range(B)]
        loader = DetBatchLoader(db, store, None, B, False, image_size=S1, device=dev)
        host_rows = np.arange(B, dtype=np.int64)
        index = torch.from_numpy(host_rows).to(dev)
        make = lambda: loader._make(host_rows, index, None)[0]                 # noqa: E731

        def step(mode, loader_fed):
            m, opt = models[mode]
            opt.zero_grad(set_to_none=True)
            out = m.detection_loss(make()) if loader_fed else m.detection_loss(imgs / 255, targets)
            sum(out.values()).backward()
            opt.step()
        legs = {"loader": lambda mode: make(), "step_loader": lambda mode: step(mode, True), "step_host": lambda mode: step(mode, False),
                "valid_loader": lambda mode: models[mode][0](make(), output="device"),
                "valid_host": lambda mode: models[mode][0](imgs / 255, output="device")}
        t = {mode: {k: [] for k in legs} for mode in MODES}
        for _ in range(ROUNDS):
            for mode in MODES:   # the modes and the legs alternate inside a round
                for name, fn in legs.items():
                    t[mode][name].append(timed(lambda: fn(mode), 2, 8))
        for mode in MODES:
            md = {k: float(np.median(v)) for k, v in t[mode].items()}
            row = dict(model="d0", batch=B, compute_dtype=mode, image_size=S1, loader_ms=md["loader"], step_loader_ms=md["step_loader"],
                       step_host_ms=md["step_host"], step_loader_over_host=md["step_loader"] / md["step_host"],
                       valid_loader_ms=md["valid_loader"], valid_host_ms=md["valid_host"],
                       valid_loader_over_host=md["valid_loader"] / md["valid_host"],
                       loader_step_within_3pct=bool(md["step_loader"] <= SLACK * md["step_host"]),
                       spread={k: [min(v), max(v)] for k, v in t[mode].items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
        for mode in MODES:
            models[mode][0]._plans.clear()
        torch.cuda.empty_cache()
    with open(os.path.join(outdir, "det_batch_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), canvas=E.MAX_SIZE, rounds=ROUNDS, images=f"{N_IMAGES} x {W}x{H}", rows=rows),
                  f, indent=1)
    slow = [(r["batch"], r["compute_dtype"], r["step_loader_over_host"]) for r in rows if not r["loader_step_within_3pct"]]
    if slow:
        print(f"GATE FAILED: the loader-fed step is more than 3 % slower than the host-fed step: {slow}", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
