#!/usr/bin/env python3
"""EfficientDet D0 / D3 on one MI355X: images/s at 512^2 for batch 1, 8 and 32 in each compute mode (fp32, bf16, f16), forward only
and end to end (uint8 images -> CPU dicts), against an eager PyTorch restatement (tests/detector_ref.eager_forward, MIOpen convs,
fp32) with the same seeded weights.  The three modes of one (model, batch) are timed in the same process, alternating, ROUNDS
times each: native_forward_ms is the median and native_forward_ms_min / _max the spread.  FLOPs and bytes come from the layer shapes
and the mode's element sizes (_Plan.flops / .bytes); the bound is max(FLOPs / MFMA peak of the mode: 157.3 TF fp32, 2516.8 TF
bf16 / f16, bytes / 6.3 TB/s measured HBM copy rate).  launches_per_forward counts kernel launches (_Plan.launches + the
preprocess).  "errors" holds, per model, 16-bit mode and output tensor, e_dev = max|device - Y| / max|Y| against the fp32
restatement Y and e_emu, the same figure of the storage-rounding emulation tests/detector16_ref.forward16 (D0 on both test
images, D3 on the first).  Usage: python tools/detector_bench.py OUTDIR -> OUTDIR/detector_bench.json (commit it as
profiles/detector_bench.json); python tools/detector_bench.py --profile [MODE]: D0 at batch 8, 20 forwards, for
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


PEAK_FLOPS, HBM_BPS = {"fp32": 157.3e12, "bf16": 2516.8e12, "f16": 2516.8e12}, 6.3e12
MAX_REL_ERR = 1e-4   # fp32 native vs eager, relative to each output's largest magnitude
MODES = ("fp32", "bf16", "f16")
ROUNDS = 3


def _model(cc, mode, dev):
    m = E.setup_detector("efficientdet", "d3" if cc else "d0", compute_dtype=mode)
    sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(sd, strict=True)
    return m.to(dev), sd


def profile(mode="fp32"):
    dev = torch.device("cuda")
    m, _ = _model(0, mode, dev)
    src = [torch.from_numpy(R.images()[i % 2]).to(dev) for i in range(8)]
    for _ in range(20):
        m.run_raw(src, 0, dev)
    torch.cuda.synchronize()


def errors(cc, models, sd):
    """e_dev and e_emu of the 16-bit modes against the fp32 restatement on the host (the end-to-end test's figures)."""
    from tests import detector16_ref as R16
    n = 1 if cc else 2
    x = R16.canvas()[:n]
    chw = [im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in R.images()[:n]]
    names = ["reg", "cls"] + [f"f{i}" for i in range(5)]
    flat = lambda o: [o[1], o[2]] + list(o[0])  # noqa: E731
    out = []
    with torch.no_grad():
        yard = flat(R.eager_forward(sd, cc, 1, x))
        for mode, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            emu = flat(R16.forward16(sd, cc, 1, x, R16.rounder(dt), dt))
            got = flat(models[mode](chw, postprocess=False))
            for nme, y, e, d in zip(names, yard, emu, got):
                out.append(dict(model=f"d{cc}", dtype=mode, tensor=nme, e_dev=R16.rel_err(d, y), e_emu=R16.rel_err(e, y)))
                print(json.dumps(out[-1]), flush=True)
    return out


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda")
    rows, errs = [], []
    ims = R.images()
    st = torch.cuda.current_stream().cuda_stream
    for cc in (0, 3):
        models = {}
        for mode in MODES:
            models[mode], sd = _model(cc, mode, dev)
        errs += errors(cc, models, sd)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        for B in (1, 8, 32):
            src = [torch.from_numpy(ims[i % 2]).to(dev) for i in range(B)]
            plans = {mode: models[mode].run_raw(src, 0, dev)[0] for mode in MODES}
            canvas = plans["fp32"].canvas.permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                _, er, ec = R.eager_forward(sdd, cc, 1, canvas)
                eager = timed(lambda: R.eager_forward(sdd, cc, 1, canvas))
            err = {mode: max(((p.reg - er).abs().max() / er.abs().max()).item(), ((p.cls - ec).abs().max() / ec.abs().max()).item())
                   for mode, p in plans.items()}
            assert err["fp32"] < MAX_REL_ERR, f"d{cc} batch {B}: native vs eager {err['fp32']:.2e}"
            fwd = {mode: [] for mode in MODES}
            for _ in range(ROUNDS):   # alternating, so that a drift of the machine meets every mode alike
                for mode in MODES:
                    fwd[mode].append(timed(lambda: plans[mode].run(st)))
            for mode in MODES:
                m, p = models[mode], plans[mode]
                t = float(np.median(fwd[mode]))
                e2e = timed(lambda: m.detect(*m.run_raw(src, 0, dev), m.threshold, m.iou_threshold), 2, 5)
                bound = 1e3 * max(p.flops / PEAK_FLOPS[mode], p.bytes / HBM_BPS)
                rows.append(dict(model=f"d{cc}", dtype=mode, batch=B, native_forward_ms=t, native_forward_ms_min=min(fwd[mode]),
                                 native_forward_ms_max=max(fwd[mode]), native_imgs_per_s=1e3 * B / t,
                                 speedup_vs_fp32=float(np.median(fwd["fp32"])) / t, eager_forward_ms=eager,
                                 eager_imgs_per_s=1e3 * B / eager, end_to_end_ms=e2e, end_to_end_imgs_per_s=1e3 * B / e2e,
                                 launches_per_forward=p.launches + 1, max_rel_err_vs_eager=err[mode], gflop=p.flops / 1e9,
                                 mbytes=p.bytes / 1e6, bound_ms=bound, share_of_bound=bound / t))
                print(json.dumps(rows[-1]), flush=True)
            for m in models.values():   # a plan owns every intermediate: free this batch size before the next
                m._plans.clear()
            del plans
        del models
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), canvas=512, rounds=ROUNDS, rows=rows, errors=errs)
    with open(os.path.join(outdir, "detector_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--profile":
        profile(*sys.argv[2:3])
    else:
        main(sys.argv[1])
