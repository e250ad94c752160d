"""GPU: the small ops of the VGG path through the C ABI, each against plain torch in high precision: stl_maxpool2x2,
stl_bilinear_nchw, stl_l1_partial / stl_l2_partial with stl_sum_partials, stl_patch3x3 (forward), stl_nchw_to_nhwc /
stl_nhwc_to_nchw, and stl_conv_forward as vgg.list_conv builds it (planned, plain source, bias + ReLU) up to 512 channels.
Every output is prefilled with NaN (every element must be written) and every op runs twice (bit-equal results).

Bounds: tests/vgg_layers_ref.py.  Ops that only move or select values are held bit for bit; arithmetic in fp32 to
e <= max(MARGIN * e32, 1e-6) with e32 the error of torch's fp32 evaluation; tensors stored in 16 bits elementwise to one
rounding of the yardstick (2**-8 |Y| for bf16, 2**-11 |Y| for f16) plus that term.  MARGIN is 8 (tests/test_detector_train_gpu.py:
sums in another order than torch's; here the reductions add n / 8 fp32 partial sums in fp64); the fp32 3x3 conv is held with
MARGIN_CONV32 = 16, for the reason given in tests/vgg_layers_ref.py (one fp32 accumulator through K = 9 * 512 products).

Measured on the MI355X, e / e32 and the largest e per op:
* stl_maxpool2x2, the layout ops, stl_patch3x3 without normalisation, the 224 -> 224 resize: bit-equal.
* stl_bilinear_nchw: 0.89 - 1.06, e <= 2.0e-5 (the fp32 source coordinate, torch's own error; the two figures above the floor
  have ratio <= 1.00).
* stl_l1_partial / stl_l2_partial + stl_sum_partials: fp32 0 - 1.53 (e <= 6.7e-8), bf16 0 - 5.28 (e <= 7.3e-8; e32 = 0 nine times):
  one rounding of the fp32 result, all below the floor.
* stl_patch3x3 with normalisation: fp32 ratio 1.00 (e <= 9.7e-8); bf16 and f16: largest |error| / allowed 0.995 / 0.99.
* stl_conv_forward with bias + ReLU: fp32 2.58 - 7.26, e <= 1.4e-6 (512 -> 512 at 20 x 14); bf16: largest |error| / allowed 0.995,
  e <= 3.5e-3.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from stlpose_amd import capi
from tests import vgg_layers_ref as L

pytestmark = pytest.mark.gpu

DT = {"fp32": (capi.F32, torch.float32), "bf16": (capi.BF16, torch.bfloat16), "f16": (capi.F16, torch.float16)}
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


def twice(fn):
    """Run an op twice onto fresh NaN-prefilled outputs; the results are bit-equal and hold no NaN."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
        assert not torch.isnan(x.double()).any(), "an element was not written"
        assert torch.equal(x, y)
    return a


# ------------------------------------------------------------------------------------------------ stl_maxpool2x2
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Cc", [8, 64, 512])
@pytest.mark.parametrize("H,W", [(8, 6), (7, 9), (33, 20), (2, 3)])
def test_maxpool2x2_is_max_pool2d(H, W, Cc, dt):
    code, td = DT[dt]
    B = 2
    g = torch.Generator().manual_seed(H * 100 + W + Cc)
    x = torch.randint(-4, 3, (B, H, W, Cc), generator=g).float()   # few levels: ties; negatives
    x[:, :2, :2, : Cc // 2] = -1 - x[:, :2, :2, : Cc // 2].abs()      # an all-negative window
    x[1] = -1 - x[1].abs()                                          # and an all-negative image
    xt = x.to(td).cuda()

    def run():
        out = torch.full((B, H // 2, W // 2, Cc), NAN, dtype=td, device="cuda")
        capi.call("stl_maxpool2x2", code, xt.data_ptr(), out.data_ptr(), B, H, W, Cc, stream())
        return out
    got = twice(run)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert (ref[1] < 0).all()
    assert torch.equal(got.cpu().float(), ref)


# ------------------------------------------------------------------------------------------------ stl_bilinear_nchw
@pytest.mark.parametrize("src,dst", [((40, 56), (224, 224)), ((300, 260), (224, 224)), ((7, 5), (224, 224)), ((224, 224), (224, 224)),
                                     ((1, 9), (8, 8))])
def test_bilinear_nchw_is_interpolate(src, dst):
    (H, W), (Ho, Wo) = src, dst
    B, Cc = 2, 3
    x = torch.rand(B, Cc, H, W, generator=torch.Generator().manual_seed(H + W))
    xc = x.cuda()

    def run():
        out = torch.full((B, Cc, Ho, Wo), NAN, device="cuda")
        capi.call("stl_bilinear_nchw", xc.data_ptr(), out.data_ptr(), B, Cc, H, W, Ho, Wo, stream())
        return out
    got = twice(run).cpu()
    if src == dst:
        assert torch.equal(got, x)
        return
    y64 = F.interpolate(x.double(), size=dst, mode="bilinear", align_corners=False)
    y32 = F.interpolate(x, size=dst, mode="bilinear", align_corners=False)
    L.hold(f"bilinear {src} -> {dst}", got, y64, y32)


# ------------------------------------------------------------------------------------------------ stl_l1_partial / stl_l2_partial / stl_sum_partials
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("op", ["stl_l1_partial", "stl_l2_partial"])
@pytest.mark.parametrize("nblk", [1, 1024])
@pytest.mark.parametrize("n", [8, 8 * 255, 8 * 257, 8 * (1024 * 256 + 3)])
def test_l1_l2_partials_and_their_sum(n, nblk, op, dt):
    code, td = DT[dt]
    g = torch.Generator().manual_seed(n % 1000 + nblk)
    a, b = (torch.randn(n, generator=g).to(td) for _ in range(2))
    ac, bc = a.cuda(), b.cuda()
    d64 = a.double() - b.double()
    d32 = a.float() - b.float()
    y64 = d64.abs().mean() if op == "stl_l1_partial" else (d64 * d64).mean()
    y32 = d32.abs().mean() if op == "stl_l1_partial" else (d32 * d32).mean()

    def run(p, q, accumulate=0, start=NAN):
        def once():
            partial = torch.full((nblk,), NAN, dtype=F64, device="cuda")
            out = torch.full((1,), start, device="cuda")
            capi.call(op, code, p.data_ptr(), q.data_ptr(), n, partial.data_ptr(), nblk, stream())
            capi.call("stl_sum_partials", partial.data_ptr(), nblk, 1.0 / n, out.data_ptr(), accumulate, stream())
            return partial, out
        return twice(once)
    partial, out = run(ac, bc)                      # accumulate 0 onto a NaN-prefilled scalar
    tag = f"{op} {dt} n {n} nblk {nblk}"
    L.hold(f"{tag} partials", partial.sum().cpu() / n, y64, y32)
    L.hold(f"{tag} sum", out[0].cpu(), y64, y32)
    _, acc = run(ac, bc, accumulate=1, start=1.5)   # accumulate 1 onto a known value
    L.hold(f"{tag} accumulated", acc[0].cpu(), y64 + 1.5, y32 + 1.5)
    zp, zero = run(ac, ac.clone())                  # identical inputs: exactly 0
    assert zero.item() == 0.0 and (zp == 0).all()


@pytest.mark.parametrize("op", ["stl_l1_partial", "stl_l2_partial"])
def test_l1_l2_partial_refuse_a_ragged_length(op):
    a = torch.ones(16, device="cuda")
    partial = torch.full((4,), NAN, dtype=F64, device="cuda")
    with pytest.raises(RuntimeError, match="n%8"):
        capi.call(op, capi.F32, a.data_ptr(), a.data_ptr(), 12, partial.data_ptr(), 4, stream())
    torch.cuda.synchronize()
    assert torch.isnan(partial).all()   # refused, not run


# ------------------------------------------------------------------------------------------------ stl_patch3x3 (forward)
@pytest.mark.parametrize("dt", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W", [(1, 7, 5), (2, 16, 12), (3, 9, 10)])
def test_patch3x3_forward_is_unfold(B, H, W, stride, norm, dt):
    code, td = DT[dt]
    img = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H * W + stride))
    ic = img.cuda()
    mean = torch.tensor([0.485, 0.456, 0.406], device="cuda")
    std = torch.tensor([0.229, 0.224, 0.225], device="cuda")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1

    def run():
        out = torch.full((B, Ho, Wo, 32), NAN, dtype=td, device="cuda")
        capi.call("stl_patch3x3", code, ic.data_ptr(), out.data_ptr(), B, H, W, stride, mean.data_ptr() if norm else None,
                  std.data_ptr() if norm else None, stream())
        return out
    got = twice(run).cpu()
    assert (got[..., 27:] == 0).all()
    got = got[..., :27]
    tag = f"patch3x3 {dt} {B}x{H}x{W} stride {stride} norm {norm}"
    if not norm:   # values are only moved: the image's own, rounded once for a 16-bit output
        assert torch.equal(got, L.unfold3x3(img, stride).to(td))
        return
    y64, y32 = L.unfold3x3(L.normalise(img, F64), stride), L.unfold3x3(L.normalise(img, F32), stride)
    if dt == "fp32":
        L.hold(tag, got, y64, y32)
    else:          # the fp32 result rounded once
        L.hold16(tag, got, y64, y32, L.ROUND[td])


# ------------------------------------------------------------------------------------------------ stl_nchw_to_nhwc / stl_nhwc_to_nchw
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Cc,H,W", [(2, 3, 5, 7), (1, 48, 9, 4)])
def test_layout_ops_are_permute(B, Cc, H, W, dt):
    code, td = DT[dt]
    x = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(Cc))
    xc = x.cuda()

    def to_nhwc(src):
        def once():
            out = torch.full((B, H, W, Cc), NAN, dtype=td, device="cuda")
            capi.call("stl_nchw_to_nhwc", code, src.data_ptr(), out.data_ptr(), B, Cc, H, W, stream())
            return out
        return twice(once)

    def to_nchw(src):
        def once():
            out = torch.full((B, Cc, H, W), NAN, device="cuda")
            capi.call("stl_nhwc_to_nchw", code, src.data_ptr(), out.data_ptr(), B, Cc, H, W, stream())
            return out
        return twice(once)
    t = to_nhwc(xc)
    assert torch.equal(t.cpu(), x.permute(0, 2, 3, 1).to(td))
    back = to_nchw(t)
    assert torch.equal(back.cpu(), x.to(td).float())
    # the round trip is the identity (on values the element type holds)
    assert torch.equal(to_nhwc(back), t) and torch.equal(to_nchw(to_nhwc(back)), back)
    # stl_nhwc_to_nchw from a tensor that stl_nchw_to_nhwc did not write
    y = torch.randn(B, H, W, Cc, generator=torch.Generator().manual_seed(Cc + 1)).to(td)
    assert torch.equal(to_nchw(y.cuda()).cpu(), y.float().permute(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ stl_conv_forward as vgg.list_conv builds it
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,Ci,Co", [(1, 20, 14, 512, 512), (2, 9, 7, 256, 512), (1, 33, 17, 64, 128), (2, 5, 4, 512, 512)])
def test_conv_bias_relu_as_the_trunk_plans_it(B, H, W, Ci, Co, dt):
    code, td = DT[dt]
    bf16 = dt == "bf16"
    g = torch.Generator().manual_seed(Ci + Co + H)
    x = F.relu(torch.randn(B, Ci, H, W, generator=g)).to(td)               # NCHW, the values the kernel reads
    w = torch.randn(Co, Ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * Ci))
    bias = torch.randn(Co, generator=g) * 0.5
    xt = x.permute(0, 2, 3, 1).contiguous().cuda()
    wt = w.permute(0, 2, 3, 1).contiguous().to(td).cuda()                   # [Co][tap][Ci], rounded as stl_weight_prep rounds
    bc = bias.cuda()

    def run():
        out = torch.full((B, H, W, Co), NAN, dtype=td, device="cuda")
        p = capi.Conv()
        p.dtype, p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co = code, B, H, W, Ci, H, W, Co
        p.ks, p.stride, p.shape = 3, 1, -1
        p.src.x, p.src.mode = xt.data_ptr(), capi.SRC_PLAIN
        p.w, p.out, p.bias, p.out_relu = wt.data_ptr(), out.data_ptr(), bc.data_ptr(), 1
        capi.call("stl_conv_plan", C.byref(p))
        capi.call("stl_conv_forward", C.byref(p), stream())
        return out
    got = twice(run).cpu().permute(0, 3, 1, 2)
    y64, y32 = L.layer(x, w, bias, False, F64, bf16), L.layer(x, w, bias, False, F32, bf16)
    assert (y64 > 0).double().mean().item() > 0.1
    tag = f"conv {dt} {B}x{H}x{W} {Ci}->{Co} ({capi.lib().stl_last_kernel().decode()})"
    if bf16:
        L.hold16(tag, got, y64, y32)
    else:
        L.hold(tag, got, y64, y32, L.MARGIN_CONV32)
