#!/usr/bin/env python3
"""Gatys stylisation benchmark (GPU only): `python tools/stylise_bench.py OUTDIR` writes OUTDIR/stylise_bench.json.

One iteration of stlpose_amd.GatysStylizer at BASELINE config 4's size (B = 16 images of 3 x 512 x 512, one 512 x 512 style
image), fp32 and bf16: the VGG19 forward up to conv5_1 with the content MSE and the Gram matrices against cached targets
(GatysStylizer.forward_loss), then the native image gradient (GatysStylizer.image_grad).  Times are device events around each
half, summed over `reps` iterations after a warm-up.  The yardstick is the same cached-target iteration written with torch
autograd of oracle.vgg_ref (cuDNN/MIOpen convolutions) on the same GPU, fp32 and under bf16 autocast.

Cost model: conv_flops = 2 x (2 x MACs of the 13 convolutions) per image (forward + the 13 data gradients); gram_flops = the
Gram matrices (2 HW C^2 per image and style tap) plus the Gram terms of the backward (the same again); bytes = every post-ReLU
map written by the forward and read back by the next layer and the backward mask, and every gradient map written and read once
(5 passes over the 13 maps, storage type).  "bound" names the larger of flops / peak and bytes / peak, "share_of_peak" is that
lower bound over the measured time; peaks from MI355X_MICROARCH.md: 157.3 TF fp32 (MFMA = vector rate), 2.5 PF bf16 MFMA dense,
8.0 TB/s HBM.
"""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {"fp32": 157.3e12, "bf16": 2.5e15}
PEAK_BW = 8.0e12
B, H, W = 16, 512, 512


def cost(dt):
    from stlpose_amd.vgg19_style import STYLE_TAPS, VGG19_LAYOUT, vgg19_flops_per_image
    conv = 2.0 * vgg19_flops_per_image(H, W) * B
    gram, maps, h, w = 0.0, 0.0, H, W
    for i, (_, _, co, pool) in enumerate(VGG19_LAYOUT):
        if pool:
            h, w = h // 2, w // 2
        maps += h * w * co
        if i in STYLE_TAPS:
            gram += 2 * (2.0 * h * w * co * co) * B
    bytes_ = 5 * maps * B * (4 if dt == "fp32" else 2)
    return conv, gram, bytes_


def rates(sec, dt):
    conv, gram, bytes_ = cost(dt)
    fl = conv + gram
    t_f, t_b = fl / PEAK[dt], bytes_ / PEAK_BW
    return {"flops": fl, "conv_flops": conv, "gram_flops": gram, "bytes": bytes_, "tflops": fl / sec / 1e12,
            "floor_compute_s": t_f, "floor_memory_s": t_b, "bound": "compute" if t_f >= t_b else "memory",
            "share_of_peak": max(t_f, t_b) / sec}


def time_halves(fwd, bwd, reps, warm):
    for _ in range(warm):
        bwd(fwd())
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record()
        r = fwd()
        e[1].record()
        bwd(r)
        e[2].record()
    torch.cuda.synchronize()
    f = sum(e[0].elapsed_time(e[1]) for e in ev) / reps * 1e-3
    b = sum(e[1].elapsed_time(e[2]) for e in ev) / reps * 1e-3
    return f, b


def native(dt, content, style, w, reps):
    from stlpose_amd import GatysStylizer
    from stlpose_amd.vgg import ready
    st = GatysStylizer(w, 1.0, 1e5, dt)
    ready(st.loss, content.device)
    it, grams = st.targets(content, style)
    img = content.clone()
    f, b = time_halves(lambda: st.forward_loss(it, img, grams)[1], lambda g: st.image_grad(it, g), reps, 2)
    return f, b


def yardstick(dt, content, style, w, reps):
    from oracle import vgg_ref
    mean = torch.tensor(vgg_ref.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(vgg_ref.IMAGENET_STD, device="cuda").view(1, 3, 1, 1)
    ac = torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == "bf16")
    with torch.no_grad(), ac:
        fc = vgg_ref.vgg19_taps((content - mean) / std, w)[vgg_ref.VGG19_CONTENT_TAP]
        fs = vgg_ref.vgg19_taps((style - mean) / std, w)
        grams = [vgg_ref.gram(fs[i].float()) for i in vgg_ref.VGG19_STYLE_TAPS]
    img = content.clone().requires_grad_(True)

    def fwd():
        with ac:
            f = vgg_ref.vgg19_taps((img - mean) / std, w)
            c = torch.nn.functional.mse_loss(f[vgg_ref.VGG19_CONTENT_TAP].float(), fc.float())
            s = sum(((vgg_ref.gram(f[i].float()) - a) ** 2).mean() for i, a in zip(vgg_ref.VGG19_STYLE_TAPS, grams))
            return c + 1e5 * s

    def bwd(loss):
        img.grad = None
        loss.backward()

    return time_halves(fwd, bwd, reps, 2)


def main(outdir):
    if not torch.cuda.is_available():
        raise SystemExit("stylise_bench: no GPU")
    from oracle import vgg_ref
    os.makedirs(outdir, exist_ok=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    content = torch.rand(B, 3, H, W, device="cuda", generator=g)
    style = torch.rand(1, 3, H, W, device="cuda", generator=g)
    w_cpu = vgg_ref.synth_vgg19_weights()
    w = {k: v.cuda() for k, v in w_cpu.items()}
    props = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
           "B": B, "H": H, "W": W, "style": [1, 3, H, W], "cases": {}}
    for dt, reps in (("fp32", 5), ("bf16", 10)):
        f, b = native(dt, content, style, w_cpu, reps)
        it = f + b
        res["cases"][f"native_{dt}"] = {"ms_per_iter": it * 1e3, "ms_forward": f * 1e3, "ms_backward": b * 1e3,
                                        "image_iters_per_s": B / it, "reps": reps, **rates(it, dt)}
        torch.cuda.empty_cache()
        f, b = yardstick(dt, content, style, w, reps)
        it_y = f + b
        res["cases"][f"torch_autograd_oracle_{dt}"] = {"ms_per_iter": it_y * 1e3, "ms_forward": f * 1e3, "ms_backward": b * 1e3,
                                                       "image_iters_per_s": B / it_y, "reps": reps, **rates(it_y, dt)}
        res["cases"][f"speedup_{dt}"] = it_y / it
        torch.cuda.empty_cache()
        print(json.dumps({k: v for k, v in res["cases"].items() if dt in k}), flush=True)
    with open(os.path.join(outdir, "stylise_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: stylise_bench.py OUTDIR")
    main(sys.argv[1])
