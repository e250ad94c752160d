#!/usr/bin/env python3
"""AdaIN stylisation benchmark (GPU only): `python tools/adain_bench.py OUTDIR` writes OUTDIR/adain_bench.json.

stlpose_amd.AdaINStylizer at BASELINE config 4's size (B = 16 content images of 3 x 512 x 512, one 512 x 512 style image), fp32
and bf16, with the style passed as an image (its encoder pass inside the call) and prepared (``prepare_style`` outside).  Times
are device events around whole calls, averaged over `reps` calls after a warm-up.  The yardstick is the same network as
``torch.nn`` modules (tests/adain_ref.py: MIOpen convolutions, ReflectionPad2d, MaxPool2d, Upsample) on the same GPU, fp32 and
under bf16 autocast.

Cost model.  conv_flops = 2 x MACs of the 9 encoder + 9 decoder convs for the B content images (plus the 9 encoder convs of the
style image when it is not prepared), stated twice: at the (h+2) x (w+2) maps the kernels run on ("padded": the ring trick's
extra work) and at the network's true sizes.  stream_bytes = what the kernels around the convs must move (input patches, every
gather's read of the previous interior and write of the padded map, the statistics' read of relu4_1, the output); each family
is also timed on its own (its launches of one call, back to back) and its bytes over that time is stated as a share of the
8.0 TB/s HBM peak.  "share_of_peak" of a whole call is the compute floor at the TRUE conv sizes over the measured time; peaks
from MI355X_MICROARCH.md: 157.3 TF fp32 (MFMA = vector rate), 2.5 PF bf16 MFMA dense, 8.0 TB/s HBM.

Accuracy of the bf16 mode (small shape, against tests/adain_ref.py in fp32 on the CPU, next to the bf16-rounded yardstick of
tests/test_adain_gpu.py) is recorded too.
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
FAMILIES = {"input": ("stl_adain_input",), "gather": ("stl_reflect_gather",), "stats": ("stl_adain_stats",), "conv": ("stl_conv_forward",)}


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / reps * 1e-3


def cost(dt, prepared):
    from stlpose_amd.adain import conv_macs, stream_bytes
    esz = 4 if dt == "fp32" else 2
    padded, true = 2.0 * conv_macs(B, H, W, True), 2.0 * conv_macs(B, H, W, False)
    by = stream_bytes(B, H, W, esz)
    if not prepared:
        padded += 2.0 * conv_macs(1, H, W, True, decode=False)
        true += 2.0 * conv_macs(1, H, W, False, decode=False)
        for k, v in stream_bytes(1, H, W, esz, decode=False).items():
            by[k] += v
    return padded, true, by


def rates(sec, dt, prepared):
    padded, true, by = cost(dt, prepared)
    return {"conv_flops_padded": padded, "conv_flops_true": true, "ring_overhead": padded / true, "stream_bytes": by,
            "tflops_true": true / sec / 1e12, "floor_compute_s": true / PEAK[dt], "floor_stream_s": sum(by.values()) / PEAK_BW,
            "share_of_peak": true / PEAK[dt] / sec}


def families(m, content, dt, reps):
    """Each kernel family of one prepared-style call, its launches run back to back: ms, and for the streaming kernels their
    bytes and share of the HBM peak."""
    from stlpose_amd import capi
    plan = m._plan(content.device, B, H, W, True)
    st = torch.cuda.current_stream().cuda_stream
    _, _, by = cost(dt, True)
    out = {}
    for fam, names in FAMILIES.items():
        ops = [lst.select(lambda n: n in names) for lst in (plan.encode, plan.decode)]
        sec = timed(lambda: [lst.run(st) for lst in ops], reps)
        out[fam] = {"launches": sum(map(len, ops)), "ms": sec * 1e3}
        if fam in by:
            out[fam].update(bytes=by[fam], tb_per_s=by[fam] / sec / 1e12, share_of_hbm_peak=by[fam] / sec / PEAK_BW)
    sec = timed(lambda: capi.call("stl_adain_output", m.dtype, plan.act.data_ptr(), plan.out.data_ptr(), B, H, W, 8, 1, st), reps)
    out["output"] = {"launches": 1, "ms": sec * 1e3, "bytes": by["output"], "tb_per_s": by["output"] / sec / 1e12,
                     "share_of_hbm_peak": by["output"] / sec / PEAK_BW}
    return out


def yardstick(dt, enc, dec, content, style, prepared, reps):
    from tests import adain_ref as R
    ac = torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == "bf16")
    with torch.no_grad(), ac:
        ms, ss = R.mean_sigma(enc(style).float())

        def call():
            with ac:
                m, s = (ms, ss) if prepared else R.mean_sigma(enc(style).float())
                fc = enc(content)
                return dec(R.adain(fc.float(), m, s, 1.0)).float().clamp(0.0, 1.0)

        return timed(call, reps)


def accuracy():
    """bf16 mode at (2,3,64,48) / style (1,3,40,56), alpha 1: error and cosine against the fp32 restatement on the CPU, next to
    the restatement with weights and stored maps rounded to bf16."""
    from stlpose_amd import AdaINStylizer
    from tests import adain_ref as R
    enc, dec = R.synth()
    g = torch.Generator().manual_seed(7)
    c, s = torch.rand(2, 3, 64, 48, generator=g), torch.rand(1, 3, 40, 56, generator=g)
    ref, yard = R.stylise(enc, dec, c, s, 1.0), R.stylise_bf16_rounded(enc, dec, c, s, 1.0)
    out = {"shape": [2, 3, 64, 48], "yardstick_bf16_rounded": {"err": R.rel_err(yard, ref), "cosine": R.cosine(yard, ref)}}
    for dt in ("fp32", "bf16"):
        got = AdaINStylizer(enc.state_dict(), dec.state_dict(), dt).stylise(c.cuda(), s.cuda(), 1.0, clamp=False).cpu()
        out[f"native_{dt}"] = {"err": R.rel_err(got, ref), "cosine": R.cosine(got, ref)}
    return out


def main(outdir):
    if not torch.cuda.is_available():
        raise SystemExit("adain_bench: no GPU")
    from stlpose_amd import AdaINStylizer
    from tests import adain_ref as R
    os.makedirs(outdir, exist_ok=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    content = torch.rand(B, 3, H, W, device="cuda", generator=g)
    style = torch.rand(1, 3, H, W, device="cuda", generator=g)
    enc_cpu, dec_cpu = R.synth()
    enc, dec = R.synth()
    enc, dec = enc.cuda(), dec.cuda()
    props = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
           "B": B, "H": H, "W": W, "style": [1, 3, H, W], "alpha": 1.0, "cases": {}, "kernel_families": {}}
    for dt, reps in (("fp32", 5), ("bf16", 10)):
        m = AdaINStylizer(enc_cpu.state_dict(), dec_cpu.state_dict(), compute_dtype=dt)
        st = m.prepare_style(style)
        for prepared in (False, True):
            tag = "prepared" if prepared else "unprepared"
            sec = timed(lambda: m.stylise(content, st if prepared else style, 1.0, True), reps)
            res["cases"][f"native_{dt}_{tag}"] = {"ms": sec * 1e3, "images_per_s": B / sec, "reps": reps, **rates(sec, dt, prepared)}
            sec_y = yardstick(dt, enc, dec, content, style, prepared, reps)
            res["cases"][f"torch_nn_{dt}_{tag}"] = {"ms": sec_y * 1e3, "images_per_s": B / sec_y, "reps": reps, **rates(sec_y, dt, prepared)}
            res["cases"][f"speedup_{dt}_{tag}"] = sec_y / sec
            print(json.dumps({k: (v if not isinstance(v, dict) else {"ms": v["ms"]}) for k, v in res["cases"].items() if dt in k and tag in k}), flush=True)
        res["kernel_families"][dt] = families(m, content, dt, reps)
        print(json.dumps(res["kernel_families"][dt]), flush=True)
        del m
        torch.cuda.empty_cache()
    res["accuracy"] = accuracy()
    with open(os.path.join(outdir, "adain_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: adain_bench.py OUTDIR")
    main(sys.argv[1])
