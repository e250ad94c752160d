#!/usr/bin/env python3
"""Fine-tuning step of the EfficientDet detector with the backbone's last stage on one MI355X (EfficientDetBackbone.detection_loss +
backward + an SGD step over detector_train.trainable_parameters), fp32, D0 and D3 at batch 8 and 32.  Two legs: "all" (every BiFPN
cell with the heads: the "all" leg of tools/detector_bifpn_bench.py) and "all" + ``set_train_backbone(max)`` (block 15 of D0, blocks
24 and 25 of D3).  One model per leg; both legs of one (model, batch) are timed in one process, alternating, ROUNDS times each,
every timing between device synchronisations (tools/detector_bench.timed); the medians are reported.

The blocks' share is the second leg minus the first (blocks_ms).  Next to it the same blocks in eager PyTorch under autograd
(tests/detector_backbone_ref.block_forward, MIOpen convs) from the block input the plan stored, differentiated from the gradient of
P5 the native backward made, with their SGD step (eager_blocks_ms); and the blocks' backward launches replayed alone, in all and by
entry point (blocks_bwd_ms, blocks_bwd_ms_by_launch).

No number is fixed in advance.  The script fails only if a result is non-finite or, with ``--baseline FILE`` (the
detector_bifpn_bench.json of the parent commit's tools/detector_bifpn_bench.py, run in the same session), if the "all" leg's step
time lies further from that file's "all" leg than that tool's own run-to-run spread (max - min over its rounds); both spreads and
the difference are recorded.

Usage: python tools/detector_backbone_bench.py OUTDIR [--baseline FILE] -> OUTDIR/detector_backbone_bench.json (commit it as
profiles/detector_backbone_bench.json)."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import detector_train as T, efficientdet as E  # noqa: E402
from stlpose_amd.launch import LaunchList  # noqa: E402
from tests import detector_backbone_ref as KR, detector_ref as R  # noqa: E402
from tools.detector_bench import timed  # noqa: E402
from tools.detector_train_bench import BOXES  # noqa: E402

ROUNDS = 3
LEGS = ("all", "all+backbone")


def main(outdir, baseline=None):
    os.makedirs(outdir, exist_ok=True)
    base = {}
    if baseline:
        with open(baseline) as f:
            base = {(r["model"], r["batch"]): r for r in json.load(f)["rows"] if r["train_bifpn"] == "all"}
    dev = torch.device("cuda")
    ims = R.images()
    rows, failures = [], []
    for cc in (0, 3):
        models = {}
        for leg in LEGS:
            m = E.setup_detector("efficientdet", "d3" if cc else "d0")
            sd = R.synth_state_dict({n: tuple(v.shape) for n, v in m.state_dict().items()})
            m.load_state_dict(sd, strict=True)
            m = m.to(dev).set_train_bifpn("all")
            if leg != "all":
                m.set_train_backbone(m.final_stage_blocks())
            models[leg] = (m, torch.optim.SGD([p for _, p in T.trainable_parameters(m)], lr=1e-5))
        kb = models[LEGS[1]][0].train_backbone
        specs = E.block_specs(cc)
        blocks = list(range(len(specs) - kb, len(specs)))
        for B in (8, 32):
            chw = torch.stack([torch.from_numpy(ims[0].transpose(2, 0, 1).astype(np.float32) / np.float32(255))] * B).to(dev)
            targets = [{"boxes": BOXES[: 1 + i % 2], "labels": torch.ones(1 + i % 2, dtype=torch.long)} for i in range(B)]
            st = torch.cuda.current_stream().cuda_stream
            losses = {}

            def train_step(leg):
                m, opt = models[leg]
                opt.zero_grad(set_to_none=True)
                loss = sum(m.detection_loss(chw, targets).values())
                loss.backward()
                opt.step()
                losses[leg] = loss.detach()
            for leg in LEGS:
                train_step(leg)
            m = models[LEGS[1]][0]
            plan = m.plan(B, dev)
            tr = plan.train
            # the blocks in eager torch: from the stored input of the first of them, against the native gradient of P5
            gp5 = tr.gp5.detach().clone().permute(0, 3, 1, 2).contiguous()
            x_in = plan.blocks[blocks[0]].inp.detach().permute(0, 3, 1, 2).contiguous()
            pre = tuple(f"{KR.PRE}{i}." for i in blocks)
            esd = {n: v.detach().clone() for n, v in m.state_dict().items() if n.startswith(pre) and v.is_floating_point()}
            for n, v in esd.items():
                v.requires_grad_(not n.endswith(("running_mean", "running_var")))
            eopt = torch.optim.SGD([v for v in esd.values() if v.requires_grad], lr=1e-5)

            def eager_step():
                eopt.zero_grad(set_to_none=True)
                x = x_in
                for i in blocks:
                    x = KR.block_forward(esd, i, specs[i], x)
                x.backward(gp5)
                eopt.step()
            blocks_bwd = LaunchList(tr.bwd.keep)
            blocks_bwd.calls = tr.bwd.calls[tr.blocks_start:]   # behind the cells': P5's data gradient and the blocks
            t = {leg: [] for leg in LEGS}
            t["eager_blocks"] = []
            for _ in range(ROUNDS):
                for leg in LEGS:   # the legs alternate inside a round
                    t[leg].append(timed(lambda: train_step(leg)))
                t["eager_blocks"].append(timed(eager_step, 2, 5))
            med = {name: float(np.median(v)) for name, v in t.items()}
            spread = {name: [min(v), max(v)] for name, v in t.items()}
            row = dict(model=f"d{cc}", batch=B, train_backbone=kb, blocks=blocks, all_step_ms=med["all"],
                       all_backbone_step_ms=med["all+backbone"], blocks_ms=med["all+backbone"] - med["all"],
                       blocks_share=(med["all+backbone"] - med["all"]) / med["all+backbone"], eager_blocks_ms=med["eager_blocks"],
                       blocks_bwd_ms=timed(lambda: blocks_bwd.run(st)),
                       blocks_bwd_ms_by_launch={name: timed(lambda s=blocks_bwd.select(lambda x, name=name: x == name): s.run(st))
                                                for name in sorted(set(blocks_bwd.names()))},
                       bwd_launches={leg: len(models[leg][0].plan(B, dev).train.bwd) for leg in LEGS}, spread=spread,
                       loss={leg: float(v) for leg, v in losses.items()})
            if (f"d{cc}", B) in base:
                b = base[f"d{cc}", B]
                bs = b["spread"]["train"]
                tol = bs[1] - bs[0]
                row.update(baseline_all_step_ms=b["train_step_ms"], baseline_spread=bs, drift_ms=med["all"] - b["train_step_ms"],
                           drift_tolerance_ms=tol)
                if abs(row["drift_ms"]) > tol:
                    failures.append(f"d{cc} batch {B}: the \"all\" leg {med['all']:.3f} ms against the baseline's {b['train_step_ms']:.3f} ms, "
                                    f"tolerance {tol:.3f} ms")
            flat = [row["all_step_ms"], row["all_backbone_step_ms"], row["eager_blocks_ms"], row["blocks_bwd_ms"], *row["loss"].values()]
            if not all(math.isfinite(v) for v in flat):
                failures.append(f"d{cc} batch {B}: a non-finite result")
            rows.append(row)
            print(json.dumps(row), flush=True)
            for leg in LEGS:
                models[leg][0]._plans.clear()
            del plan, tr, blocks_bwd, esd, x_in, gp5
            torch.cuda.empty_cache()
    with open(os.path.join(outdir, "detector_backbone_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), canvas=512, rounds=ROUNDS, compute_dtype="fp32", baseline=bool(base),
                       failures=failures, rows=rows), f, indent=1)
    for msg in failures:
        print("FAIL", msg, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    base_file = args[args.index("--baseline") + 1] if "--baseline" in args else None
    sys.exit(main(args[0], base_file))
