#!/usr/bin/env python3
"""Fine-tuning step of the EfficientDet heads on one MI355X (EfficientDetBackbone.detection_loss + backward + an SGD step over
regressor.* / classifier.*), D0 and D3 at batch 8 and 32, compute_dtype "fp32" and "f16" (f16 forward, bf16 gradients), next to
(a) the inference forward alone (_Plan.run) and (b), for fp32, the same head-only step with the heads in eager PyTorch under
autograd (tests/detector_train_ref.heads_forward, MIOpen convs) on the features the plan produced -- (b) takes its loss and output
gradients from the same stl_det_loss launch, so it times the heads' forward, backward and the optimiser step, not the frozen
trunk.  Everything of one (model, batch) is timed in one process, the two modes alternating, ROUNDS times each; the medians, the
heads' share train_step - trunk (for f16 it holds the host's wait for the non-finite check of reg / cls) and the ratios train_step /
forward, eager_heads_step / heads' share and f16 / fp32 are reported.  One gate: at batch 32 the f16 step must be faster than the
fp32 step of the same run (the 16-bit trunk alone saves more than the heads could lose unless the 16-bit backward is slower than
the fp32 one); each batch-32 f16 row records it as "f16_step_below_fp32", and the tool exits with status 1, after writing the
file, if one is false.  The heads' share against fp32's is reported, not gated.  Usage: python tools/detector_train_bench.py
OUTDIR -> OUTDIR/detector_train_bench.json (commit it as profiles/detector_train_bench.json)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import efficientdet as E  # noqa: E402
from tests import detector_ref as R, detector_train_ref as TR  # noqa: E402
from tools.detector_bench import timed  # noqa: E402

ROUNDS = 3
MODES = ("fp32", "f16")
BOXES = torch.tensor([[60.0, 40.0, 180.0, 160.0], [230.0, 110.0, 330.0, 290.0]])


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda")
    ims = R.images()
    rows = []
    for cc in (0, 3):
        models = {}
        for mode in MODES:
            m = E.setup_detector("efficientdet", "d3" if cc else "d0", compute_dtype=mode)
            sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
            m.load_state_dict(sd, strict=True)
            m = m.to(dev)
            heads = [p for k, p in m.named_parameters() if k.startswith(("regressor.", "classifier."))]
            models[mode] = (m, torch.optim.SGD(heads, lr=1e-5))
        for B in (8, 32):
            chw = torch.stack([torch.from_numpy(ims[0].transpose(2, 0, 1).astype(np.float32) / np.float32(255))] * B).to(dev)
            targets = [{"boxes": BOXES[: 1 + i % 2], "labels": torch.ones(1 + i % 2, dtype=torch.long)} for i in range(B)]
            st = torch.cuda.current_stream().cuda_stream

            def train_step(mode):
                m, opt = models[mode]
                opt.zero_grad(set_to_none=True)
                sum(m.detection_loss(chw, targets).values()).backward()
                opt.step()
            plans = {}
            for mode in MODES:
                train_step(mode)
                plans[mode] = models[mode][0].plan(B, dev)
            m, p = models["fp32"][0], plans["fp32"]
            feats = [f.permute(0, 3, 1, 2).contiguous() for f, _ in p.feats]
            esd = TR.head_state(m.state_dict(), torch.float32)
            esd = {k: v.detach().to(dev).requires_grad_(v.requires_grad) for k, v in esd.items()}
            eopt = torch.optim.SGD([v for v in esd.values() if v.requires_grad], lr=1e-5)
            gt, off = tr_gt(m, targets, chw, dev)

            def eager_step():
                eopt.zero_grad(set_to_none=True)
                reg, cls = TR.heads_forward(esd, cc, 1, feats)
                _, dreg, dlogit, _ = torch.ops.stlpose.det_loss(reg.detach(), cls.detach(), m._anchor_dev, gt, off, 0.25, 2.0, 50.0)
                pd = cls.detach()
                torch.autograd.backward([reg, cls], [dreg, dlogit / (pd * (1 - pd)).clamp(min=1e-30)])
                eopt.step()
            t = {mode: {"forward": [], "trunk": [], "train": []} for mode in MODES}
            t["fp32"]["eager"] = []
            for _ in range(ROUNDS):
                for mode in MODES:   # the modes alternate inside a round
                    q = plans[mode]
                    t[mode]["forward"].append(timed(lambda: q.run(st)))
                    t[mode]["trunk"].append(timed(lambda: q.run(st, upto=q.head_start)))
                    t[mode]["train"].append(timed(lambda: train_step(mode)))
                t["fp32"]["eager"].append(timed(eager_step, 2, 5))
            med = {mode: {k: float(np.median(v)) for k, v in t[mode].items()} for mode in MODES}
            for mode in MODES:
                md, tr = med[mode], plans[mode].train
                row = dict(model=f"d{cc}", batch=B, compute_dtype=mode, forward_ms=md["forward"], trunk_ms=md["trunk"],
                           train_step_ms=md["train"], train_step_over_forward=md["train"] / md["forward"],
                           native_heads_step_ms=md["train"] - md["trunk"])
                if mode == "fp32":
                    row.update(eager_heads_step_ms=md["eager"], eager_over_native_heads_step=md["eager"] / (md["train"] - md["trunk"]))
                else:
                    f32 = med["fp32"]
                    row.update(train_step_over_fp32=md["train"] / f32["train"],
                               heads_step_over_fp32=(md["train"] - md["trunk"]) / (f32["train"] - f32["trunk"]))
                    if B == 32:
                        row.update(f16_step_below_fp32=bool(md["train"] < f32["train"]))
                row.update(spread={k: [min(v), max(v)] for k, v in t[mode].items()}, fwd_launches=len(tr.fwd), bwd_launches=len(tr.bwd))
                rows.append(row)
                print(json.dumps(row), flush=True)
            for mode in MODES:
                models[mode][0]._plans.clear()
            del p, plans, feats, esd
            torch.cuda.empty_cache()
    with open(os.path.join(outdir, "detector_train_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), canvas=512, rounds=ROUNDS, rows=rows), f, indent=1)
    slow = [(r["model"], r["train_step_ms"]) for r in rows if r.get("f16_step_below_fp32") is False]
    if slow:
        print(f"GATE FAILED: the f16 step is not faster than the fp32 step at batch 32: {slow}", flush=True)
        return 1
    return 0


def tr_gt(m, targets, chw, dev):
    from stlpose_amd.detector_train import pack_targets
    gt, off = pack_targets(targets, [tuple(c.shape[1:]) for c in chw], m.num_classes)
    return torch.from_numpy(gt).to(dev), torch.from_numpy(off).to(dev)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
