"""GPU: the split-bf16 conv mode (``stl_conv.math = STL_MATH_BF16X3``, ``compute_dtype="fp32x3"``).

Per launch through the C ABI: the device lies within ``bound`` of the three-term product summed in fp64 (tests/split_ref.py: Y and
the bound, MARGIN x the fp32 conv's own error on the same operands -- tests/test_fp32x3_cpu.py shows that the bound holds for
the three products in fp32 and fails for plain fp32 and for two products), the native launch on the same operands lies outside
it (so the mode is on), and two launches agree bit for bit.  Whole nets at the bars of the fp32 tests they mirror
(tests/test_hrnet_gpu.py, tests/test_vgg_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import hrnet_ref, vgg_ref  # noqa: E402  (checker only)
from stlpose_amd import PoseHighResolutionNet, VGGPerceptualLoss, capi, forward_pass, get_max_preds_hrnet  # noqa: E402
from tests.golden.make_golden import synth_batch  # noqa: E402
from tests.split_ref import LAUNCH_CASES, bound_for, case_tensors, launch_case  # noqa: E402

EPS = 1e-5


def stream():
    return torch.cuda.current_stream().cuda_stream


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def conv_desc(x, w, stride, math, dtype=None):
    """(descriptor, the device tensors it points into, output) of a conv of NCHW x with OIHW w; planned as the engine plans."""
    B, Ci, H, W = x.shape
    Co, _, ks, _ = w.shape
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xt, wt = nhwc(x), nhwc(w)   # [B][H][W][Ci], [Co][tap][Ci]
    out = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
    p = capi.Conv()
    p.dtype = capi.F32 if dtype is None else dtype
    p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co, p.ks, p.stride, p.shape = B, H, W, Ci, Ho, Wo, Co, ks, stride, -1
    p.math = math
    p.src.x, p.src.mode = xt.data_ptr(), capi.SRC_PLAIN
    p.w, p.out = wt.data_ptr(), out.data_ptr()
    return p, [xt, wt], out


def launch(p, out):
    capi.call("stl_conv_plan", C.byref(p))
    capi.call("stl_conv_forward", C.byref(p), stream())
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).double().cpu()


def check(name, y, bound, run):
    """run(math) -> NCHW fp64 on the host.  The three assertions of a launch."""
    d1, d1b, d0 = run(capi.MATH_BF16X3), run(capi.MATH_BF16X3), run(capi.MATH_NATIVE)
    scale = float(y.abs().max())
    e1, e0, d10 = float((d1 - y).abs().max()) / scale, float((d0 - y).abs().max()) / scale, float((d1 - d0).abs().max()) / scale
    print(f"{name}: bound {bound:.3e}; math=1 {e1 / bound:.3f} x, math=0 {e0 / bound:.2f} x from Y; math=1 from math=0 {d10 / bound:.2f} x")
    assert not torch.isnan(d1).any() and not torch.isnan(d0).any()
    assert e1 <= bound, f"{name}: {e1:.3e} of max |Y| from the three-term product, bound {bound:.3e}"
    assert d10 > bound, f"{name}: the math = 1 launch is within {d10:.3e} of the native one: the mode is not on"
    assert torch.equal(d1, d1b), f"{name}: two math = 1 launches differ"
    return d1, d0


@pytest.mark.parametrize("name", [c[0] for c in LAUNCH_CASES])
def test_launch_plain(name):
    x, w, stride, padding, y, bound = launch_case(name)

    def run(math):
        p, keep, out = conv_desc(x, w, stride, math)
        return launch(p, out)
    check(name, y, bound, run)


def _bn_transform(x, gamma, beta, mean, var):
    """relu(a x + b) as the kernel forms it: a = gamma * rstd, b = fma(-mean, a, beta), v = fma(a, x, b), each rounded once to fp32."""
    rstd = (1.0 / torch.sqrt((var + EPS).double())).float()
    a = gamma * rstd
    b = (beta.double() - mean.double() * a.double()).float()
    v = (a.double().view(1, -1, 1, 1) * x.double() + b.double().view(1, -1, 1, 1)).float()
    return torch.relu(v)


@pytest.mark.parametrize("name", ["c32", "deep"])
def test_launch_bn_source_on_running_statistics(name):
    x0, w, stride, padding = case_tensors(name)
    Ci = x0.shape[1]
    g = torch.Generator().manual_seed(5)
    x = 1.5 * torch.randn(x0.shape, generator=g) + 0.3   # a raw conv output: the BatchNorm + ReLU is applied on load
    gamma, beta = torch.rand(Ci, generator=g) + 0.5, 0.2 * torch.randn(Ci, generator=g)
    mean, var = 0.1 * torch.randn(Ci, generator=g), torch.rand(Ci, generator=g) * 0.8 + 0.8
    y, bound = bound_for(_bn_transform(x, gamma, beta, mean, var), w, stride, padding)

    def run(math):
        p, keep, out = conv_desc(x, w, stride, math)
        dev = [t.cuda() for t in (gamma, beta, mean, var)]
        p.src.mode, p.src.relu, p.src.eps, p.src.inv_count = capi.SRC_BN, 1, EPS, 1.0 / (x.shape[0] * x.shape[2] * x.shape[3])
        p.src.gamma, p.src.beta, p.src.rmean, p.src.rvar = (t.data_ptr() for t in dev)
        return launch(p, out)
    check(name + " BN source", y, bound, run)


@pytest.mark.parametrize("name", ["stem", "deep"])
def test_launch_bias_and_relu(name):
    x, w, stride, padding = case_tensors(name)
    bias = 0.05 * torch.randn(w.shape[0], generator=torch.Generator().manual_seed(6))
    y, bound = bound_for(x, w, stride, padding, bias, relu=True)

    def run(math):
        p, keep, out = conv_desc(x, w, stride, math)
        b = bias.cuda()
        p.bias, p.out_relu = b.data_ptr(), 1
        return launch(p, out)
    check(name + " bias + ReLU", y, bound, run)


def test_launch_block_end_source():
    """STL_SRC_BNADD with src_out: the stored block-end sum does not see the split; the conv over it meets the bound."""
    B, H, W, Cc = 2, 12, 9, 64
    g = torch.Generator().manual_seed(11)
    yraw, skip = 1.5 * torch.randn(B, Cc, H, W, generator=g) + 0.3, torch.relu(torch.randn(B, Cc, H, W, generator=g))
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, 0.2 * torch.randn(Cc, generator=g)
    mean, var = 0.1 * torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) * 0.8 + 0.8
    w = torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (Cc * 9)) ** 0.5
    res = {}
    for math in (capi.MATH_NATIVE, capi.MATH_BF16X3, capi.MATH_BF16X3):
        p, keep, out = conv_desc(yraw, w, 1, math)
        dev = [t.cuda() for t in (gamma, beta, mean, var)]
        st, z = nhwc(skip), torch.full((B, H, W, Cc), float("nan"), device="cuda")
        capi.call("stl_conv_plan", C.byref(p))
        assert capi.lib().stl_conv_bnadd_ok(C.byref(p)) == 1
        p.src.mode, p.src.relu, p.src.eps, p.src.inv_count, p.src.y = capi.SRC_BNADD, 1, EPS, 1.0 / (B * H * W), st.data_ptr()
        p.src.gamma, p.src.beta, p.src.rmean, p.src.rvar = (t.data_ptr() for t in dev)
        p.src_out = z.data_ptr()
        capi.call("stl_conv_forward", C.byref(p), stream())
        torch.cuda.synchronize()
        res.setdefault(math, []).append((z.cpu(), out.permute(0, 3, 1, 2).double().cpu()))
    (z0, o0), = res[capi.MATH_NATIVE]
    (z1, o1), (z1b, o1b) = res[capi.MATH_BF16X3]
    assert not torch.isnan(z0).any() and torch.equal(z0, z1), "the stored block-end sum depends on math"
    assert torch.equal(o1, o1b) and torch.equal(z1, z1b)
    y, bound = bound_for(z0.permute(0, 3, 1, 2).contiguous(), w, 1, 1)
    scale = float(y.abs().max())
    e1, d10 = float((o1 - y).abs().max()) / scale, float((o1 - o0).abs().max()) / scale
    print(f"block end: bound {bound:.3e}; math=1 {e1 / bound:.3f} x from Y; math=1 from math=0 {d10 / bound:.2f} x")
    assert e1 <= bound and d10 > bound


def test_math_with_other_dtype_or_data_gradient_is_an_error():
    x, w, stride, padding = case_tensors("c32")
    lib = capi.lib()
    p, keep, out = conv_desc(x.to(torch.bfloat16), w.to(torch.bfloat16), stride, capi.MATH_BF16X3, dtype=capi.BF16)
    for fn in (lambda: lib.stl_conv_plan(C.byref(p)), lambda: lib.stl_conv_forward(C.byref(p), stream())):
        assert fn() != 0 and b"math" in lib.stl_last_error() and b"dtype" in lib.stl_last_error()
    q, keep2, out2 = conv_desc(x, w, stride, capi.MATH_BF16X3)
    q.src.mode = capi.SRC_BNBWD
    for fn in (lambda: lib.stl_conv_plan(C.byref(q)), lambda: lib.stl_conv_forward(C.byref(q), stream())):
        assert fn() != 0 and b"math" in lib.stl_last_error() and b"BNBWD" in lib.stl_last_error()
    r, keep3, out3 = conv_desc(x, w, stride, 2)
    assert lib.stl_conv_forward(C.byref(r), stream()) != 0 and b"math" in lib.stl_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(out2).all() and torch.isnan(out3).all(), "an error case launched"


# ---------------------------------------------------------------------------------------- whole nets
def _load_synth(model):
    sd = {k: torch.from_numpy(hrnet_ref.synth_tensor(k, tuple(v.shape))) for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    return model


def test_tiny_eval_vs_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_tiny_eval.npz"))
    m = _load_synth(PoseHighResolutionNet("tiny", "fp32x3")).cuda().eval()
    with torch.no_grad():
        out = m(torch.from_numpy(g["img"]).cuda()).cpu().numpy()
    err = np.abs(out - g["output"]).max() / np.abs(g["output"]).max()
    print(f"tiny eval fp32x3 vs G1: {err:.3e} of max")
    assert err < 1e-3, f"eval output rel err {err}"


def test_w32_flip_test_vs_reference_golden_and_vs_fp32(golden_dir):
    g = np.load(os.path.join(golden_dir, "g3_w32_256x192.npz"))
    img, _, _ = synth_batch(2, 256, 192, seed=1234, sigma=2.0)
    outs = {}
    for dt in ("fp32x3", "fp32"):
        m = _load_synth(PoseHighResolutionNet("w32", dt)).cuda().eval()
        with torch.no_grad():
            outs[dt] = forward_pass(m, torch.from_numpy(img).cuda(), "HRNet", device="cuda", flip=True).cpu().numpy()
    ref = g["flip_sample"]
    scale = np.abs(ref).max()
    e3, e1 = (np.abs(outs[dt].reshape(-1)[::64] - ref).max() / scale for dt in ("fp32x3", "fp32"))
    p3, _ = get_max_preds_hrnet(outs["fp32x3"])
    p1, _ = get_max_preds_hrnet(outs["fp32"])
    print(f"W32 256x192 flip test vs G3: fp32x3 {e3:.3e}, fp32 {e1:.3e} of max; fp32x3 from fp32 {np.abs(outs['fp32x3'] - outs['fp32']).max() / scale:.3e}")
    assert e3 < 1e-3
    assert np.array_equal(p3, g["flip_argmax_xy"]), "flip-test argmax differs from the reference"
    assert np.array_equal(p3, p1), "argmax differs from the fp32 mode's"
    assert not np.array_equal(outs["fp32x3"], outs["fp32"]), "the two modes computed the same bits: the mode is not on"


def test_w48_eval_vs_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g8_w48.npz"))
    m = _load_synth(PoseHighResolutionNet("w48", "fp32x3")).cuda().eval()
    img, _, _ = synth_batch(1, 128, 96, seed=5)
    with torch.no_grad():
        o = m(torch.from_numpy(img).cuda()).cpu().numpy()
    ref = g["out_sample"]
    err = np.abs(o.reshape(-1)[::16] - ref).max() / np.abs(ref).max()
    print(f"W48 eval fp32x3 vs G8: {err:.3e} of max")
    assert err < 1e-3


def test_inf_in_the_image_gives_non_finite_heat_maps_in_both_modes(golden_dir):
    """One Inf in the input image gives non-finite heat maps in both modes, so that Evaluator's finiteness check fires.

    The convs carry it (Inf * w = +-Inf, sums of both signs NaN; the split form keeps the Inf in lo) and the ReLU of the fp32
    kernels keeps a NaN as torch's does (common.cuh, max_lo).  With fmaxf for the ReLU, as before this mode, the NaN that conv2
    makes of conv1's +-Inf channels was zeroed by the next ReLU and 0 of 6528 heat-map values were non-finite in either mode."""
    g = np.load(os.path.join(golden_dir, "g1_tiny_eval.npz"))
    img = torch.from_numpy(g["img"]).clone()
    img[0, 1, img.shape[2] // 2, img.shape[3] // 2] = float("inf")
    outs = {}
    for dt in ("fp32x3", "fp32"):
        m = _load_synth(PoseHighResolutionNet("tiny", dt)).cuda().eval()
        with torch.no_grad():
            outs[dt] = m(img.cuda()).cpu()
        print(f"Inf in image 0, {dt}: {int((~torch.isfinite(outs[dt][0])).sum())} of {outs[dt][0].numel()} heat-map values of image 0 non-finite, "
              f"{int((~torch.isfinite(outs[dt][1:])).sum())} of the other images'")
    for dt, out in outs.items():
        assert not bool(torch.isfinite(out[0]).all()), dt
        assert bool(torch.isfinite(out[1:]).all()), dt   # the other images of the batch are untouched


def test_launch_inf_operand_is_non_finite_like_the_native_launch():
    """An Inf (a NaN) among a launch's operands: the outputs it reaches are +-Inf (NaN) exactly where, and with the signs, the
    native launch gives them -- hi is rounded from the clamped value, so the Inf is carried by lo instead of becoming
    Inf - Inf -- and every other output is untouched."""
    x, w, stride, padding, y, bound = launch_case("c32")
    clean = None
    for bad in (None, float("inf"), float("-inf"), float("nan")):
        xb = x.clone()
        if bad is not None:
            xb[1, 3, 5, 4] = bad
        res = {}
        for math in (capi.MATH_BF16X3, capi.MATH_NATIVE):
            p, keep, out = conv_desc(xb, w, stride, math)
            res[math] = launch(p, out)
        d1, d0 = res[capi.MATH_BF16X3], res[capi.MATH_NATIVE]
        if bad is None:
            clean = d1
            assert bool(torch.isfinite(d1).all())
            continue
        hit = ~torch.isfinite(d0)
        assert int(hit.sum()) == 9 * w.shape[0] and bool(hit[1, :, 4:7, 3:6].all())   # the 3 x 3 window, every channel
        assert torch.equal(~torch.isfinite(d1), hit), bad
        assert torch.equal(torch.nan_to_num(d1[hit], nan=0.5), torch.nan_to_num(d0[hit], nan=0.5)), bad   # Inf signs, NaN as NaN
        assert torch.equal(d1[~hit], clean[~hit]), bad


def test_gradients_are_refused(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_tiny_eval.npz"))
    img = torch.from_numpy(g["img"]).cuda()
    m = _load_synth(PoseHighResolutionNet("tiny", "fp32x3")).cuda()
    m.train()
    with pytest.raises(NotImplementedError, match='compute_dtype="fp32"'):
        m(img)
    m.eval()
    with pytest.raises(NotImplementedError, match="third bf16 piece"):
        m(img.clone().requires_grad_())
    with torch.no_grad():   # ... and neither left anything behind
        assert bool(torch.isfinite(m(img)).all())
    from stlpose_amd.trainer import Trainer
    exp = {"training": {"num_epochs": 1, "save_frequency": 1}, "dataset": {"image_size": [64, 64]}}
    with pytest.raises(NotImplementedError, match='compute_dtype="fp32"'):
        Trainer("/nonexistent", exp, [], [], 2, arch="tiny", compute_dtype="fp32x3")


@pytest.mark.parametrize("tag", ["rs_rgb", "rs_gray", "nr_rgb", "nr_odd", "nr_gray"])
def test_vgg_matches_reference_fixture_g10(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "g10_vgg.npz"))
    a, b = torch.from_numpy(g[f"{tag}_in"]).cuda(), torch.from_numpy(g[f"{tag}_tg"]).cuda()
    got = {}
    for dt in ("fp32x3", "fp32"):
        m = VGGPerceptualLoss(resize=bool(g[f"{tag}_resize"]), state_dict=vgg_ref.synth_vgg_weights(), compute_dtype=dt).cuda()
        got[dt] = m(a, b).item()
    ref = float(g[f"{tag}_loss"])
    print(f"VGG16 perceptual loss {tag} vs G10: fp32x3 {abs(got['fp32x3'] - ref) / abs(ref):.3e}, fp32 {abs(got['fp32'] - ref) / abs(ref):.3e} relative")
    assert abs(got["fp32x3"] - ref) <= 1e-3 * abs(ref), (tag, got, ref)
