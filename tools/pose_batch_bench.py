#!/usr/bin/env python3
"""Batch-building benchmark (GPU only): `python tools/pose_batch_bench.py OUTDIR [--batches N] [--steps K]` writes
OUTDIR/pose_batch_bench.json.

Workload: HRNet-W32, mixed, 384 x 288, batches of 32; N x 32 synthetic persons over 256 synthetic resident images of 640 x 480, the
reference's augmentation settings (scale_factor 0.35, rot_factor 45, flip, half body above 8 joints with probability 0.3).  All
legs run in one process, alternating (a, b, c-loader, c-fixed, a, b, ...), the device synchronised before and after each; a figure is
the median of its 3 runs.
  loader_ms_per_batch        (a) PoseBatchLoader + ResidentImages alone: one epoch of N batches, wall time / N.
  host_path_ms_per_batch     (b) the same batches by the host path: per person half_body_transform and the draws in Python,
                             augment.crop_batch with its upload of the batch's images, transform_joints per person, generate_targets.
  step_loader_ms             (c) TrainStep fed by the loader (load_batch + step per batch), wall time per step, against
  step_fixed_ms              the same TrainStep stepping on one fixed batch (bench.py's measurement).
  loader_launches_ms         device time of the loader's launches for one batch (pose_augment, the two table gathers, affine_crop,
                             gaussian_targets, the joint-weight multiply), from device events; median of 5.
The script fails when (a) is not below (b).
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

EXP = {"dataset": {"scale_factor": 0.35, "rot_factor": 45.0, "flip": True, "num_joints_half_body": 8, "prob_half_body": 0.3}}


def synthetic_db(n_persons, n_images, h, w, size, seed=0):
    from stlpose_amd.pose_data import PersonDB, xywh2cs
    rng = np.random.default_rng(seed)
    image_index = np.sort(rng.integers(0, n_images, n_persons)).astype(np.int64)
    joints = np.zeros((n_persons, 17, 3))
    x0, y0 = rng.uniform(0, w * 0.5, n_persons), rng.uniform(0, h * 0.4, n_persons)
    bw, bh = rng.uniform(60, w * 0.45, n_persons), rng.uniform(120, h * 0.55, n_persons)
    joints[:, :, 0] = np.round(x0[:, None] + rng.uniform(0, 1, (n_persons, 17)) * bw[:, None])
    joints[:, :, 1] = np.round(y0[:, None] + rng.uniform(0, 1, (n_persons, 17)) * bh[:, None])
    seen = rng.uniform(0, 1, (n_persons, 17)) < 0.8
    joints[~seen] = 0
    vis = np.zeros((n_persons, 17, 3))
    vis[:, :, 0] = vis[:, :, 1] = seen
    cs = [xywh2cs(x0[i], y0[i], bw[i], bh[i], size[0] / size[1]) for i in range(n_persons)]
    return PersonDB(joints=joints, joints_vis=vis, center=np.stack([c for c, _ in cs]), scale=np.stack([s for _, s in cs]),
                    image_index=image_index, image_id=image_index + 1, width=np.full(n_persons, w, np.int32),
                    height=np.full(n_persons, h, np.int32), score=np.ones(n_persons), alpha=np.zeros(n_persons),
                    perceptual_loss=np.zeros(n_persons), images=[dict(id=k + 1, file_name=f"{k}.jpg", width=w, height=h) for k in range(n_images)],
                    image_size=size)


def host_batch(db, images, rows, rng, size, weight, dev):
    """One training batch the way the package offered it before the loader: JointsDataset.py:164-200 per person on the host."""
    from stlpose_amd.augment import crop_batch, half_body_transform, transform_joints
    from stlpose_amd.targets import generate_targets
    ds = EXP["dataset"]
    sf, rf = ds["scale_factor"], ds["rot_factor"]
    centers, scales, rots, flips = [], [], [], []
    for i in rows:
        c, s, r = db.center[i], db.scale[i], 0.0
        if np.sum(db.joints_vis[i][:, 0]) > ds["num_joints_half_body"] and rng.random() < ds["prob_half_body"]:
            ch, sh = half_body_transform(db.joints[i], db.joints_vis[i], size[0] / size[1], rng=_Randn(rng))
            if ch is not None:
                c, s = ch, sh
        s = s.astype(np.float64) * np.clip(rng.standard_normal() * sf + 1, 1 - sf, 1 + sf)
        if rng.random() <= 0.6:
            r = float(np.clip(rng.standard_normal() * rf, -rf * 2, rf * 2))
        centers.append(c), scales.append(s), rots.append(r), flips.append(bool(ds["flip"] and rng.random() <= 0.5))
    imgs, trans = crop_batch([images[int(k)] for k in db.image_index[rows]], centers, scales, rots, flips, size, device=dev)
    jv = [transform_joints(db.joints[i], db.joints_vis[i], trans[b], flips[b], int(db.width[i])) for b, i in enumerate(rows)]
    target, tw = generate_targets(torch.from_numpy(np.stack([j for j, _ in jv])), torch.from_numpy(np.stack([v for _, v in jv])),
                                  (size[0] // 4, size[1] // 4), size, 2.0, device=dev)
    return imgs, target, tw * weight


class _Randn:
    def __init__(self, rng):
        self.rng = rng

    def randn(self):
        return self.rng.standard_normal()


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


def main(outdir, batches, steps, batch=32, H=384, W=288, n_images=256, ih=480, iw=640):
    if not torch.cuda.is_available():
        raise SystemExit("pose_batch_bench: no GPU")
    from bench import synth_batch
    from stlpose_amd import PoseBatchLoader, PoseHighResolutionNet, ResidentImages
    from stlpose_amd.pose_data import JOINTS_WEIGHT
    from stlpose_amd.train_step import TrainStep
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda:0")
    load0 = os.getloadavg()[0]
    size = (W, H)
    db = synthetic_db(batches * batch, n_images, ih, iw, size)
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (ih, iw, 3), dtype=torch.uint8, generator=g) for _ in range(n_images)]
    store = ResidentImages.from_arrays([im.numpy() for im in images], dev)
    loader = PoseBatchLoader(db, store, EXP, batch, True, seed=0, device=dev)
    weight = torch.tensor(JOINTS_WEIGHT, device=dev).view(1, 17, 1)
    torch.manual_seed(0)
    model = PoseHighResolutionNet("w32", "mixed").to(dev)
    ts = TrainStep(model, batch, H, W, optimizer="adam", lr=1e-3, device=dev)
    fixed = synth_batch(batch, H, W, 0, dev, sigma=3.0)

    def leg_loader():
        n = 0
        for _ in loader:
            n += 1
        return n

    def leg_host():
        rng = np.random.default_rng(1)
        rows_all = np.random.default_rng(2).permutation(len(db))
        for b in range(batches):
            host_batch(db, images, rows_all[b * batch:(b + 1) * batch], rng, size, weight, dev)
        return batches

    def leg_step_loader():
        n = 0
        for imgs, target, tw, _ in loader:
            ts.load_batch(imgs, target, tw)
            ts.step()
            n += 1
            if n >= steps:
                break
        return n

    def leg_step_fixed():
        ts.load_batch(*fixed)
        for _ in range(steps):
            ts.step()
        return steps
    legs = {"loader": leg_loader, "host_path": leg_host, "step_loader": leg_step_loader, "step_fixed": leg_step_fixed}
    for fn in legs.values():   # warm-up: plans, lazy kernel attributes, allocator
        fn()
    times = {k: [] for k in legs}
    for _ in range(3):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / n * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}

    it = iter(loader)
    launches_ms = events(lambda: next(it))
    res = {"device": torch.cuda.get_device_name(0),
           "workload": f"HRNet-W32 mixed {H}x{W} bs={batch}; {len(db)} persons over {n_images} resident images of {iw}x{ih} "
                       f"({store.nbytes / 2 ** 20:.0f} MiB); {batches} batches per epoch, {steps} steps per step leg",
           "loader_ms_per_batch": med["loader"], "host_path_ms_per_batch": med["host_path"],
           "step_loader_ms": med["step_loader"], "step_fixed_ms": med["step_fixed"],
           "loader_adds_to_step_ms": med["step_loader"] - med["step_fixed"],
           "loader_images_per_s": batch / med["loader"] * 1e3, "host_path_images_per_s": batch / med["host_path"] * 1e3,
           "loader_launches_ms": launches_ms, "runs_ms": times,
           "loadavg": {"before": load0, "after": os.getloadavg()[0], "cpus": os.cpu_count()}}
    with open(os.path.join(outdir, "pose_batch_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not med["loader"] < med["host_path"]:
        raise SystemExit("pose_batch_bench: the loader is not faster than the host path")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="batch-building benchmark")
    ap.add_argument("outdir")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    main(a.outdir, a.batches, a.steps)
