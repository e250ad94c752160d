#!/usr/bin/env python3
"""Fine-tuning step of the EfficientDet heads on one MI355X (EfficientDetBackbone.detection_loss + backward + an SGD step over
regressor.* / classifier.*), D0 and D3 at batch 8 and 32, fp32, next to (a) the inference forward alone (_Plan.run) and (b) the
same head-only step with the heads in eager PyTorch under autograd (tests/detector_train_ref.heads_forward, MIOpen convs) on the
features the plan produced -- (b) takes its loss and output gradients from the same stl_det_loss launch, so it times the heads'
forward, backward and the optimiser step, not the frozen trunk.  The three are timed in one process, alternating, ROUNDS times
each; the medians and the ratios train_step / forward and eager_heads_step / (train_step - trunk) are reported, no threshold is
set.  Usage: python tools/detector_train_bench.py OUTDIR -> OUTDIR/detector_train_bench.json (commit it as
profiles/detector_train_bench.json)."""
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
BOXES = torch.tensor([[60.0, 40.0, 180.0, 160.0], [230.0, 110.0, 330.0, 290.0]])


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda")
    ims = R.images()
    rows = []
    for cc in (0, 3):
        m = E.setup_detector("efficientdet", "d3" if cc else "d0")
        sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        heads = [p for k, p in m.named_parameters() if k.startswith(("regressor.", "classifier."))]
        opt = torch.optim.SGD(heads, lr=1e-5)
        for B in (8, 32):
            chw = torch.stack([torch.from_numpy(ims[0].transpose(2, 0, 1).astype(np.float32) / np.float32(255))] * B).to(dev)
            targets = [{"boxes": BOXES[: 1 + i % 2], "labels": torch.ones(1 + i % 2, dtype=torch.long)} for i in range(B)]
            st = torch.cuda.current_stream().cuda_stream

            def train_step():
                opt.zero_grad(set_to_none=True)
                sum(m.detection_loss(chw, targets).values()).backward()
                opt.step()
            train_step()
            p = m.plan(B, dev)
            tr = p.train
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
            t = {"forward": [], "trunk": [], "train": [], "eager": []}
            for _ in range(ROUNDS):
                t["forward"].append(timed(lambda: p.run(st)))
                t["trunk"].append(timed(lambda: p.run(st, upto=p.head_start)))
                t["train"].append(timed(train_step))
                t["eager"].append(timed(eager_step, 2, 5))
            med = {k: float(np.median(v)) for k, v in t.items()}
            rows.append(dict(model=f"d{cc}", batch=B, forward_ms=med["forward"], trunk_ms=med["trunk"], train_step_ms=med["train"],
                             eager_heads_step_ms=med["eager"], train_step_over_forward=med["train"] / med["forward"],
                             native_heads_step_ms=med["train"] - med["trunk"],
                             eager_over_native_heads_step=med["eager"] / (med["train"] - med["trunk"]),
                             spread={k: [min(v), max(v)] for k, v in t.items()}, fwd_launches=len(tr.fwd), bwd_launches=len(tr.bwd)))
            print(json.dumps(rows[-1]), flush=True)
            m._plans.clear()
            del p, tr, feats, esd
            torch.cuda.empty_cache()
    with open(os.path.join(outdir, "detector_train_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), canvas=512, rounds=ROUNDS, rows=rows), f, indent=1)


def tr_gt(m, targets, chw, dev):
    from stlpose_amd.detector_train import pack_targets
    gt, off = pack_targets(targets, [tuple(c.shape[1:]) for c in chw], m.num_classes)
    return torch.from_numpy(gt).to(dev), torch.from_numpy(off).to(dev)


if __name__ == "__main__":
    main(sys.argv[1])
