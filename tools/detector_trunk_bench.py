#!/usr/bin/env python3
"""Fine-tuning step of the EfficientDet detector with the backbone on one MI355X (EfficientDetBackbone.detection_loss + backward + an
SGD step over detector_train.trainable_parameters), fp32, D0 and D3 at batch 8 and 32.  Four legs, every BiFPN cell training in each:
"final" (``set_train_backbone(final_stage_blocks())``: the parent's configuration, the "all+backbone" leg of
tools/detector_backbone_bench.py), "half" (``set_train_trunk(n // 2)``), "blocks" (``set_train_trunk(n)``: every block) and "all"
(``set_train_trunk("all")``: the stem too).  One model per leg; the legs of one (model, batch) are timed in one process, alternating,
ROUNDS times each, every timing between device synchronisations (tools/detector_bench.timed); the medians are reported.

The trunk's share of a leg is its step minus the "final" leg's, over its step (trunk_share).  Next to it the same blocks (and the
stem) in eager PyTorch under autograd (tests/detector_trunk_ref.block_forward / stem_forward, MIOpen convs) from the maps the plan
stored -- each block from its own stored input, differentiated from the gradient of its output the native backward made
(``tr.block_dy``) -- with their SGD step (eager_ms, for the "all" leg's blocks), and the trunk's backward launches replayed alone, in all
and by entry point.

The two new depthwise kernels alone, at the largest shape of each (k, s) among the blocks of the model at that batch: time, bytes
moved (every tensor read or written once) over time, and that against tools/hbm_ceiling.py's figure for a plain fp32 copy of a tensor
far larger than the Infinity Cache (``hbm_ceiling.ceiling``, called in the same process); at k = 3, s = 1 also the heads' 3 x 3
kernels on the same tensors.

No number is fixed in advance.  The script fails only if a result is non-finite.  With ``--baseline FILE`` (the
detector_backbone_bench.json of the parent commit's tools/detector_backbone_bench.py, run in the same session) the "final" leg is
reported beside that file's "all+backbone" leg with both spreads (drift_ms, drift_tolerance_ms = that tool's max - min).

Usage: python tools/detector_trunk_bench.py OUTDIR [--baseline FILE] [--models 0,3] [--batches 8,32] -> OUTDIR/detector_trunk_bench.json
(commit it as profiles/detector_trunk_bench.json)."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import capi, detector_train as T, efficientdet as E  # noqa: E402
from stlpose_amd.launch import LaunchList  # noqa: E402
from tests import detector_ref as R, detector_trunk_ref as UR  # noqa: E402
from tools import hbm_ceiling  # noqa: E402
from tools.detector_bench import timed  # noqa: E402
from tools.detector_train_bench import BOXES  # noqa: E402

ROUNDS = 3
LEGS = ("final", "half", "blocks", "all")


def kernels_alone(specs, plan, B, ceiling, st):
    """The two new depthwise kernels at the largest (h_in^2 mid) of each (k, s)."""
    dev, lib, out = plan.dev, capi.lib(), []
    for k, s in ((3, 1), (3, 2), (5, 1), (5, 2)):
        cand = [(plan.blocks[i].inp.shape[1] ** 2 * b["mid"], i) for i, b in enumerate(specs) if (b["k"], b["s"]) == (k, s)]
        if not cand:
            continue
        _, i = max(cand)
        h, c = plan.blocks[i].inp.shape[1], specs[i]["mid"]
        ho = (h + s - 1) // s
        x, z, dx = (torch.randn(B, h, h, c, device=dev) for _ in range(3))
        dy, w, dw = torch.randn(B, ho, ho, c, device=dev), torch.randn(k, k, c, device=dev), torch.empty(k, k, c, device=dev)
        part = torch.empty(lib.stl_det_dwconv_bwd_ks_parts(B * ho * ho) * k * k * c, device=dev)
        p = [t.data_ptr() for t in (x, z, dx, dy, w, dw, part)]
        row = dict(k=k, s=s, block=i, B=B, h=h, C=c)
        ms = timed(lambda: capi.call("stl_det_dwconv_bwd_data_ks", p[3], p[4], p[1], p[2], B, h, h, c, k, s, st))
        nbytes = 4 * (dy.numel() + z.numel() + dx.numel())
        row.update(data_ms=ms, data_tbps=nbytes / ms / 1e9, data_of_copy=nbytes / ms / 1e9 / ceiling)
        ms = timed(lambda: capi.call("stl_det_dwconv_bwd_weight_ks", p[0], p[3], p[6], p[5], B, h, h, c, k, s, st))
        nbytes = 4 * (x.numel() + dy.numel())
        row.update(weight_ms=ms, weight_tbps=nbytes / ms / 1e9, weight_of_copy=nbytes / ms / 1e9 / ceiling)
        if (k, s) == (3, 1):   # the heads' kernels on the same tensors
            part9 = torch.empty(lib.stl_det_dwconv_bwd_parts(B * h * h) * 9 * c, device=dev)
            row["old_data_ms"] = timed(lambda: capi.call("stl_det_dwconv_bwd_data", p[3], p[4], p[1], p[2], B, h, h, c, st))
            row["old_weight_ms"] = timed(lambda: capi.call("stl_det_dwconv_bwd_weight", p[0], p[3], part9.data_ptr(), p[5], B, h, h, c, st))
        out.append(row)
        del x, z, dx, dy, part
    return out


def main(outdir, baseline=None, models=(0, 3), batches=(8, 32)):
    os.makedirs(outdir, exist_ok=True)
    base = {}
    if baseline:
        with open(baseline) as f:
            base = {(r["model"], r["batch"]): r for r in json.load(f)["rows"]}
    dev = torch.device("cuda")
    ims = R.images()
    ceiling = hbm_ceiling.ceiling(torch.float32, "copy")   # TB/s of a 2 GiB fp32 copy_, 1 read + 1 write
    rows, failures = [], []
    for cc in models:
        specs = E.block_specs(cc)
        nb = len(specs)
        legs = {}
        for leg in LEGS:
            m = E.setup_detector("efficientdet", "d3" if cc else "d0")
            sd = R.synth_state_dict({n: tuple(v.shape) for n, v in m.state_dict().items()})
            m.load_state_dict(sd, strict=True)
            m = m.to(dev).set_train_bifpn("all")
            if leg == "final":
                m.set_train_backbone(m.final_stage_blocks())
            else:
                m.set_train_trunk({"half": nb // 2, "blocks": nb, "all": "all"}[leg])
            legs[leg] = (m, torch.optim.SGD([p for _, p in T.trainable_parameters(m)], lr=1e-5))
        for B in batches:
            chw = torch.stack([torch.from_numpy(ims[0].transpose(2, 0, 1).astype(np.float32) / np.float32(255))] * B).to(dev)
            targets = [{"boxes": BOXES[: 1 + i % 2], "labels": torch.ones(1 + i % 2, dtype=torch.long)} for i in range(B)]
            st = torch.cuda.current_stream().cuda_stream
            losses = {}

            def train_step(leg):
                m, opt = legs[leg]
                opt.zero_grad(set_to_none=True)
                loss = sum(m.detection_loss(chw, targets).values())
                loss.backward()
                opt.step()
                losses[leg] = loss.detach()
            for leg in LEGS:
                train_step(leg)
            m = legs["all"][0]
            plan = m.plan(B, dev)
            tr = plan.train
            # the trunk in eager torch: every block from its own stored input against the native gradient of its output
            nchw = lambda t: t.detach().clone().permute(0, 3, 1, 2).contiguous()  # noqa: E731
            esd = {n: v.detach().clone() for n, v in m.state_dict().items() if n.startswith("backbone_net.") and v.is_floating_point()}
            for n, v in esd.items():
                v.requires_grad_(not n.endswith(("running_mean", "running_var")))
            eopt = torch.optim.SGD([v for v in esd.values() if v.requires_grad], lr=1e-5)
            canvas, stem_dy = nchw(plan.canvas), nchw(tr.stem_dy)

            def eager_step():
                eopt.zero_grad(set_to_none=True)
                for i in range(nb - 1, -1, -1):   # one block's maps at a time
                    UR.block_forward(esd, i, specs[i], nchw(plan.blocks[i].inp)).backward(nchw(tr.block_dy[i]))
                UR.stem_forward(esd, canvas).backward(stem_dy)
                eopt.step()
            trunk_bwd = LaunchList(tr.bwd.keep)
            trunk_bwd.calls = tr.bwd.calls[tr.blocks_start:]   # behind the cells': P5's data gradient, the blocks, the stem
            t = {leg: [] for leg in LEGS}
            t["eager"] = []
            for _ in range(ROUNDS):
                for leg in LEGS:   # the legs alternate inside a round
                    t[leg].append(timed(lambda: train_step(leg)))
                t["eager"].append(timed(eager_step, 1, 3))
            med = {name: float(np.median(v)) for name, v in t.items()}
            spread = {name: [min(v), max(v)] for name, v in t.items()}
            row = dict(model=f"d{cc}", batch=B, blocks={leg: legs[leg][0].train_backbone for leg in LEGS},
                       step_ms={leg: med[leg] for leg in LEGS},
                       trunk_ms={leg: med[leg] - med["final"] for leg in LEGS[1:]},
                       trunk_share={leg: (med[leg] - med["final"]) / med[leg] for leg in LEGS[1:]},
                       eager_ms=med["eager"], trunk_bwd_ms=timed(lambda: trunk_bwd.run(st)),
                       trunk_bwd_ms_by_launch={name: timed(lambda s=trunk_bwd.select(lambda x, name=name: x == name): s.run(st))
                                               for name in sorted(set(trunk_bwd.names()))},
                       bwd_launches={leg: len(legs[leg][0].plan(B, dev).train.bwd) for leg in LEGS}, spread=spread,
                       loss={leg: float(v) for leg, v in losses.items()})
            row["kernels"] = kernels_alone(specs, plan, B, ceiling, st)
            if (f"d{cc}", B) in base:
                b = base[f"d{cc}", B]
                bs = b["spread"]["all+backbone"]
                row.update(baseline_final_step_ms=b["all_backbone_step_ms"], baseline_spread=bs,
                           drift_ms=med["final"] - b["all_backbone_step_ms"], drift_tolerance_ms=bs[1] - bs[0])
            flat = [*row["step_ms"].values(), row["eager_ms"], row["trunk_bwd_ms"], *row["loss"].values()]
            if not all(math.isfinite(v) for v in flat):
                failures.append(f"d{cc} batch {B}: a non-finite result")
            rows.append(row)
            print(json.dumps(row), flush=True)
            for leg in LEGS:
                legs[leg][0]._plans.clear()
            del plan, tr, trunk_bwd, esd, canvas, stem_dy
            torch.cuda.empty_cache()
        del legs
        torch.cuda.empty_cache()
    with open(os.path.join(outdir, "detector_trunk_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), canvas=512, rounds=ROUNDS, compute_dtype="fp32", baseline=bool(base),
                       copy_tbps=ceiling, failures=failures, rows=rows), f, indent=1)
    for msg in failures:
        print("FAIL", msg, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default  # noqa: E731
    sys.exit(main(args[0], opt("--baseline", None), tuple(int(v) for v in opt("--models", "0,3").split(",")),
                  tuple(int(v) for v in opt("--batches", "8,32").split(","))))
