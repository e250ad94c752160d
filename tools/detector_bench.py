#!/usr/bin/env python3
"""EfficientDet D0 / D3 on one MI355X: images/s at 512^2 for batch 1, 8 and 32, forward only and end to end (uint8 images ->
CPU dicts), against an eager PyTorch restatement (tests/detector_ref.eager_forward, MIOpen convs) with the same seeded weights.
FLOPs and bytes come from the layer shapes (_Plan.flops / .bytes); the bound is max(FLOPs / 157.3 TF fp32 MFMA peak, bytes /
6.3 TB/s measured HBM copy rate).  Usage: python tools/detector_bench.py OUTDIR -> OUTDIR/detector_bench.json (commit it as
profiles/detector_bench.json); python tools/detector_bench.py --profile: D0 at batch 8, 20 forwards, for
rocprofv3 --kernel-trace --stats."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stlpose_amd import efficientdet as E  # noqa: E402
from tests import detector_ref as R  # noqa: E402


def timed(fn, warm=3, iters=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


PEAK_FLOPS, HBM_BPS = 157.3e12, 6.3e12
MAX_REL_ERR = 1e-4   # native vs eager, relative to each output's largest magnitude


def profile():
    dev = torch.device("cuda")
    m = E.setup_detector("efficientdet", "d0")
    m.load_state_dict(R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    m = m.to(dev)
    src = [torch.from_numpy(R.images()[i % 2]).to(dev) for i in range(8)]
    for _ in range(20):
        m.run_raw(src, 0, dev)
    torch.cuda.synchronize()


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda")
    rows = []
    ims = R.images()
    for cc in (0, 3):
        m = E.setup_detector("efficientdet", "d3" if cc else "d0")
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = R.synth_state_dict(shapes)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        for B in (1, 8, 32):
            src = [torch.from_numpy(ims[i % 2]).to(dev) for i in range(B)]
            p, metas = m.run_raw(src, 0, dev)
            canvas = p.canvas.permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                _, er, ec = R.eager_forward(sdd, cc, 1, canvas)
            err = max(((p.reg - er).abs().max() / er.abs().max()).item(), ((p.cls - ec).abs().max() / ec.abs().max()).item())
            assert err < MAX_REL_ERR, f"d{cc} batch {B}: native vs eager {err:.2e}"
            st = torch.cuda.current_stream().cuda_stream
            fwd = timed(lambda: p.run(st))
            with torch.no_grad():
                eager = timed(lambda: R.eager_forward(sdd, cc, 1, canvas))
            e2e = timed(lambda: m.detect(*m.run_raw(src, 0, dev), m.threshold, m.iou_threshold), 2, 5)
            rows.append(dict(model=f"d{cc}", batch=B, native_forward_ms=fwd, native_imgs_per_s=1e3 * B / fwd, eager_forward_ms=eager,
                             eager_imgs_per_s=1e3 * B / eager, end_to_end_ms=e2e, end_to_end_imgs_per_s=1e3 * B / e2e,
                             launches_per_forward=len(p.calls) + 1, max_rel_err_vs_eager=err, gflop=p.flops / 1e9,
                             mbytes=p.bytes / 1e6, bound_ms=1e3 * max(p.flops / PEAK_FLOPS, p.bytes / HBM_BPS),
                             share_of_bound=1e3 * max(p.flops / PEAK_FLOPS, p.bytes / HBM_BPS) / fwd))
            print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), canvas=512, rows=rows)
    with open(os.path.join(outdir, "detector_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--profile":
        profile()
    else:
        main(sys.argv[1])
