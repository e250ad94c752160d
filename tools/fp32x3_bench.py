#!/usr/bin/env python3
"""fp32x3 benchmark (GPU only): `python tools/fp32x3_bench.py OUTDIR` writes OUTDIR/fp32x3_bench.json.

What `compute_dtype="fp32x3"` (fp32 tensors, every conv launch multiplying split bf16 operands on the 16-bit matrix cores,
stl_conv.math = STL_MATH_BF16X3) buys over "fp32" and costs against the 16-bit modes:
  * HRNet W32 eval forward, batch 32, at 384x288 and at 256x192: fp32, fp32x3, mixed;
  * the Evaluator's flip-test batch (forward_pass(flip=True): the images and their mirrors) at 384x288: fp32, fp32x3;
  * VGG16 perceptual loss, 16 pairs at 512 x 512, resize=False: fp32, fp32x3, bf16.
The legs of a group alternate in one process; a leg's time is the median of 3 rounds, each the mean of `iters` calls between two
device events after a warm-up, the device synchronised around it.  Beside each fp32x3 time stand its error and fp32's against
the fp64 oracle (oracle/hrnet_ref.py, oracle/vgg_ref.py in double precision on the host) on one small batch, outside the timed
region: max |out - ref| / max |ref| for the heat maps, |loss - ref| / |ref| for the loss.

The script FAILS (exit status 1, after writing the file) if fp32x3 is not faster than fp32 on the W32 384x288 forward or on the
VGG16 leg.  "mfma_cycles_per_slice_implied" is what the ratio says about the matrix step if the kernels were bound by it alone:
a 64-byte K slice is four v_mfma_f32_16x16x4_f32 (4 x 32 = 128 cycles) natively and three v_mfma_f32_16x16x16_bf16 split, so
128 / ratio is an UPPER bound of three of those (the split's vector instructions and everything else are in it too).
"""
from __future__ import annotations

import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 3


def time_legs(legs, iters, warm=2):
    """legs: {name: callable}.  -> {name: median over ROUNDS of the mean seconds per call}; the legs alternate within a round."""
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e-3 / iters)
    return {k: statistics.median(v) for k, v in times.items()}, times


def load_synth(model):
    from oracle import hrnet_ref
    sd = {k: torch.from_numpy(hrnet_ref.synth_tensor(k, tuple(v.shape))) for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    return model


def hrnet_group(H, W, B, dtypes, flip, iters):
    from oracle import hrnet_ref, pose_ref
    from stlpose_amd import PoseHighResolutionNet, forward_pass
    from tests.golden.make_golden import synth_batch
    img = torch.from_numpy(synth_batch(B, H, W, seed=7)[0]).cuda()
    models = {dt: load_synth(PoseHighResolutionNet("w32", dt)).cuda().eval() for dt in dtypes}

    def leg(m):
        def run():
            with torch.no_grad():
                return forward_pass(m, img, "HRNet", device="cuda", flip=True) if flip else m(img)
        return run
    med, raw = time_legs({dt: leg(m) for dt, m in models.items()}, iters)
    # error against the fp64 oracle on the first image
    small = img[:1]
    ref_net = hrnet_ref.load_synth(hrnet_ref.RefPoseNet("w32")).double().eval()
    with torch.no_grad():
        ref = (pose_ref.forward_pass(ref_net, small.cpu().double(), flip=True) if flip else ref_net(small.cpu().double())).numpy()
    out = {}
    for dt, m in models.items():
        with torch.no_grad():
            o = (forward_pass(m, small, "HRNet", device="cuda", flip=True) if flip else m(small)).double().cpu().numpy()
        out[dt] = {"ms": med[dt] * 1e3, "images_per_s": B / med[dt], "ms_rounds": [t * 1e3 for t in raw[dt]],
                   "max_err_vs_fp64": float(np.abs(o - ref).max() / np.abs(ref).max()),
                   "argmax_differing_vs_fp64": int((o.reshape(o.shape[0], o.shape[1], -1).argmax(-1) != ref.reshape(ref.shape[0], ref.shape[1], -1).argmax(-1)).sum())}
    del models
    torch.cuda.empty_cache()
    return out


def vgg_group(iters):
    from oracle import vgg_ref
    from stlpose_amd import VGGPerceptualLoss
    w = vgg_ref.synth_vgg_weights()
    g = torch.Generator().manual_seed(16)
    a = torch.rand(16, 3, 512, 512, generator=g)
    b = (a + 0.2 * torch.randn(16, 3, 512, 512, generator=g)).clamp_(0, 1)
    ac, bc = a.cuda(), b.cuda()
    models = {dt: VGGPerceptualLoss(resize=False, state_dict=w, compute_dtype=dt).cuda() for dt in ("fp32", "fp32x3", "bf16")}
    med, raw = time_legs({dt: (lambda m=m: m(ac, bc)) for dt, m in models.items()}, iters)
    sa, sb = a[:1, :, :256, :256].contiguous(), b[:1, :, :256, :256].contiguous()   # the error: one 256 x 256 pair
    with torch.no_grad():
        ref = vgg_ref.vgg_perceptual_loss(sa.double(), sb.double(), {k: v.double() for k, v in w.items()}, resize=False).item()
    out = {}
    for dt, m in models.items():
        got = m(sa.cuda(), sb.cuda()).item()
        out[dt] = {"ms": med[dt] * 1e3, "pairs_per_s": 16 / med[dt], "ms_rounds": [t * 1e3 for t in raw[dt]], "loss_err_vs_fp64": abs(got - ref) / abs(ref)}
    return out


def main(outdir):
    if not torch.cuda.is_available():
        raise SystemExit("fp32x3_bench: no GPU")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    os.makedirs(outdir, exist_ok=True)
    props = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
           "rounds": ROUNDS, "cases": {}}
    c = res["cases"]
    c["w32_384x288_b32_forward"] = hrnet_group(384, 288, 32, ("fp32", "fp32x3", "mixed"), False, 5)
    print(json.dumps(c["w32_384x288_b32_forward"]), flush=True)
    c["w32_256x192_b32_forward"] = hrnet_group(256, 192, 32, ("fp32", "fp32x3", "mixed"), False, 10)
    print(json.dumps(c["w32_256x192_b32_forward"]), flush=True)
    c["w32_384x288_b32_flip_test"] = hrnet_group(384, 288, 32, ("fp32", "fp32x3"), True, 3)
    print(json.dumps(c["w32_384x288_b32_flip_test"]), flush=True)
    c["vgg16_perceptual_16x512x512"] = vgg_group(3)
    print(json.dumps(c["vgg16_perceptual_16x512x512"]), flush=True)
    ratio = {k: v["fp32"]["ms"] / v["fp32x3"]["ms"] for k, v in c.items()}
    res["speedup_fp32x3_over_fp32"] = ratio
    res["mfma_cycles_per_slice_implied"] = {k: 128.0 / r for k, r in ratio.items()}
    ok = ratio["w32_384x288_b32_forward"] > 1.0 and ratio["vgg16_perceptual_16x512x512"] > 1.0
    res["fp32x3_faster_than_fp32"] = ok
    with open(os.path.join(outdir, "fp32x3_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"speedup_fp32x3_over_fp32": ratio, "ok": ok}))
    if not ok:
        raise SystemExit("fp32x3_bench: fp32x3 is not faster than fp32 on the W32 384x288 forward and the VGG16 leg")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: fp32x3_bench.py OUTDIR")
    main(sys.argv[1])
