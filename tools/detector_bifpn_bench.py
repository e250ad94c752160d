#!/usr/bin/env python3
"""Fine-tuning step of the EfficientDet heads with the last k BiFPN cells on one MI355X (EfficientDetBackbone.detection_loss +
backward + an SGD step over detector_train.trainable_parameters), fp32, D0 and D3 at batch 8 and 32, k = 0 (the heads alone: the
step tools/detector_train_bench.py times), 1, the model's maximum (cells - 1) and "all" (every cell: the first one with its 1x1
layers on the backbone maps and its two plain pools).  One model per k; everything of one (model,
batch) is timed in one process, the legs alternating, ROUNDS times each, every timing between device synchronisations
(tools/detector_bench.timed); the medians are reported.

Next to each leg the same trainable part in eager PyTorch under autograd (tests/detector_bifpn_ref.cell_forward with torch's own
max-pool, tests/detector_train_ref.heads_forward, MIOpen convs) on the maps the plan produced, with the loss and output gradients
of the same stl_det_loss launch: it times forward, backward and optimiser step of the trainable part, not the frozen trunk.  The
cells' share is a leg minus the k = 0 leg, native (cells_ms) and eager (eager_cells_ms); the first cell's share is the "all" leg
minus the k = cells - 1 leg (first_cell_ms, eager_first_cell_ms: tests/detector_bifpn_first_ref.cell0_forward from the plan's P3 /
P4 / P5); at batch 32, for the largest k and for "all", the cells'
backward launches are also timed by entry point (cells_bwd_ms_by_launch: each sub-list replayed alone).

Usage: python tools/detector_bifpn_bench.py OUTDIR -> OUTDIR/detector_bifpn_bench.json (commit it as
profiles/detector_bifpn_bench.json)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import detector_train as T, efficientdet as E  # noqa: E402
from stlpose_amd.launch import LaunchList  # noqa: E402
from tests import detector_bifpn_first_ref as FR, detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR  # noqa: E402
from tools.detector_bench import timed  # noqa: E402
from tools.detector_train_bench import BOXES, tr_gt  # noqa: E402

ROUNDS = 3
LEVEL_NODES = ("conv3_up", "conv4_down", "conv5_down", "conv6_down", "conv7_down")


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda")
    ims = R.images()
    rows = []
    for cc in (0, 3):
        ks = (0, 1, E.FPN_REPEATS[cc] - 1, "all")
        models = {}
        for k in ks:
            m = E.setup_detector("efficientdet", "d3" if cc else "d0")
            sd = R.synth_state_dict({n: tuple(v.shape) for n, v in m.state_dict().items()})
            m.load_state_dict(sd, strict=True)
            m = m.to(dev).set_train_bifpn(k)
            models[k] = (m, torch.optim.SGD([p for _, p in T.trainable_parameters(m)], lr=1e-5))
        for B in (8, 32):
            chw = torch.stack([torch.from_numpy(ims[0].transpose(2, 0, 1).astype(np.float32) / np.float32(255))] * B).to(dev)
            targets = [{"boxes": BOXES[: 1 + i % 2], "labels": torch.ones(1 + i % 2, dtype=torch.long)} for i in range(B)]
            st = torch.cuda.current_stream().cuda_stream

            def train_step(k):
                m, opt = models[k]
                opt.zero_grad(set_to_none=True)
                sum(m.detection_loss(chw, targets).values()).backward()
                opt.step()
            plans = {}
            for k in ks:
                train_step(k)
                plans[k] = models[k][0].plan(B, dev)
            eager = {}
            for k in ks:   # the trainable part in eager torch, from the maps the plan of this k made
                m, p = models[k][0], plans[k]
                n = len(p.cells)
                nk = n if k == "all" else k
                cells = list(range(n - nk, n))
                if k == "all":   # from the backbone's maps
                    ins = [f.permute(0, 3, 1, 2).contiguous() for f in p.backbone]
                else:
                    ins = [p.cells[n - k - 1][name].y.permute(0, 3, 1, 2).contiguous() for name in LEVEL_NODES]
                esd = BR.train_state(m.state_dict(), cells, torch.float32)
                esd = {name: v.detach().to(dev).requires_grad_(v.requires_grad) for name, v in esd.items()}
                eopt = torch.optim.SGD([v for v in esd.values() if v.requires_grad], lr=1e-5)
                gt, off = tr_gt(m, targets, chw, dev)

                def eager_step(m=m, cells=cells, ins=ins, esd=esd, eopt=eopt, gt=gt, off=off):
                    eopt.zero_grad(set_to_none=True)
                    levels = ins
                    for j in cells:
                        if j == 0:
                            levels = BR.levels_of(FR.cell0_forward(esd, *levels, pool=lambda name, t: R._pool(t)))
                        else:
                            levels = BR.levels_of(BR.cell_forward(esd, j, levels, pool=lambda name, t: R._pool(t)))
                    reg, cls = TR.heads_forward(esd, cc, 1, levels)
                    _, dreg, dlogit, _ = torch.ops.stlpose.det_loss(reg.detach(), cls.detach(), m._anchor_dev, gt, off, 0.25, 2.0, 50.0)
                    pd = cls.detach()
                    torch.autograd.backward([reg, cls], [dreg, dlogit / (pd * (1 - pd)).clamp(min=1e-30)])
                    eopt.step()
                eager[k] = eager_step
            t = {k: {"trunk": [], "train": [], "eager": []} for k in ks}
            for _ in range(ROUNDS):
                for k in ks:   # the legs alternate inside a round
                    q = plans[k]
                    t[k]["trunk"].append(timed(lambda: q.run(st, upto=q.head_start)))
                    t[k]["train"].append(timed(lambda: train_step(k)))
                    t[k]["eager"].append(timed(eager[k], 2, 5))
            med = {k: {name: float(np.median(v)) for name, v in t[k].items()} for k in ks}
            for k in ks:
                md, tr = med[k], plans[k].train
                row = dict(model=f"d{cc}", batch=B, train_bifpn=k, trunk_ms=md["trunk"], train_step_ms=md["train"],
                           native_trainable_step_ms=md["train"] - md["trunk"], eager_trainable_step_ms=md["eager"],
                           eager_over_native_trainable_step=md["eager"] / (md["train"] - md["trunk"]))
                if k:
                    cells_ms, eager_cells_ms = md["train"] - med[0]["train"], md["eager"] - med[0]["eager"]
                    row.update(cells_ms=cells_ms, eager_cells_ms=eager_cells_ms, eager_cells_over_native=eager_cells_ms / cells_ms)
                    if k == "all":
                        first_ms, eager_first_ms = md["train"] - med[ks[-2]]["train"], md["eager"] - med[ks[-2]]["eager"]
                        row.update(first_cell_ms=first_ms, eager_first_cell_ms=eager_first_ms, eager_first_cell_over_native=eager_first_ms / first_ms)
                    if B == 32 and k in ks[-2:]:
                        first = tr.bwd.names().index("stl_det_grad_add")   # the heads' launches come first
                        cells_bwd = LaunchList(tr.bwd.keep)
                        cells_bwd.calls = tr.bwd.calls[first:]
                        row.update(cells_bwd_ms_by_launch={name: timed(lambda s=cells_bwd.select(lambda x, name=name: x == name): s.run(st))
                                                           for name in sorted(set(cells_bwd.names()))},
                                   cells_bwd_ms=timed(lambda: cells_bwd.run(st)))
                row.update(spread={name: [min(v), max(v)] for name, v in t[k].items()}, fwd_launches=len(tr.fwd), bwd_launches=len(tr.bwd))
                rows.append(row)
                print(json.dumps(row), flush=True)
            for k in ks:
                models[k][0]._plans.clear()
            del plans, eager, esd, ins, p
            torch.cuda.empty_cache()
    with open(os.path.join(outdir, "detector_bifpn_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), canvas=512, rounds=ROUNDS, compute_dtype="fp32", rows=rows), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
