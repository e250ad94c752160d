"""GPU: the detector's 16-bit compute modes (bf16, f16).  Kernel level: each *16 entry point of csrc/detector.hip against torch in
fp64 on the same 16-bit-rounded inputs, so that fp32 accumulation and one output rounding are the only error left.  End to end:
the device against the fp32 yardstick detector_ref.eager_forward, held to twice the error of the storage-rounding emulation
tests/detector16_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, efficientdet as E
from tests import detector16_ref as R16
from tests import detector_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "detector", "g15_effdet.npz")
DEV = "cuda"
DT = {"bf16": (torch.bfloat16, 1, 2.0 ** -8), "f16": (torch.float16, 2, 2.0 ** -11)}   # torch dtype, STL_* code, unit roundoff
MODES = ["bf16", "f16"]


@pytest.fixture(scope="module")
def g():
    return np.load(FIX)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _layout(g, cc):
    rows = bytes(g[f"d{cc}_layout"]).decode().split("\n")
    return {k: tuple(int(v) for v in s.split(",") if v) for k, s in (r.split(" ") for r in rows)}


def _bound(out, ref, u, what=""):
    """|out - ref| <= u |ref| + 1e-5 max|ref| (u = 0 for an fp32 output), ref in fp64."""
    out, ref = out.double().cpu(), ref.double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    mx = ref.abs().max().item()
    excess = ((out - ref).abs() - (u * ref.abs() + 1e-5 * mx)).max().item()
    print(f"{what} max|err| {(out - ref).abs().max().item():.3e} max|ref| {mx:.3e} worst excess over the bound {excess:.3e}")
    assert excess <= 0, (what, excess, mx)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ kernels
def _dwconv16(mode, xn, wk, bias, k, s, act, pool):
    dt, code, _ = DT[mode]
    B, H, W, Cc = xn.shape
    Ho, Wo = -(-H // s), -(-W // s)
    out = torch.full((B, Ho, Wo, Cc), float("nan"), device=DEV, dtype=dt)
    nparts = capi.lib().stl_det_dw16_parts(Ho * Wo)
    part = torch.full((B, nparts, Cc), float("nan"), device=DEV) if pool else None
    capi.call("stl_det_dwconv16", code, xn.data_ptr(), wk.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(),
              None if part is None else part.data_ptr(), B, H, W, Cc, k, s, act, _st())
    return out, part


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("full", [True, False], ids=["bias_swish", "plain"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("hw", [(17, 12), (16, 9)])
def test_dwconv16_and_pool_partials(mode, full, k, s, hw):
    dt, _, u = DT[mode]
    for Cc in (24, 40):
        torch.manual_seed(k * 10 + s + Cc)
        x = torch.randn(2, Cc, *hw, device=DEV).to(dt)
        w = torch.randn(Cc, 1, k, k, device=DEV)
        bias = torch.randn(Cc, device=DEV) if full else None
        ref = F.conv2d(R._same(x.double(), k, s), w.double(), None if bias is None else bias.double(), s, 0, 1, Cc)
        if full:
            ref = F.silu(ref)
        wk = w[:, 0].permute(1, 2, 0).contiguous()
        out, part = _dwconv16(mode, _nhwc(x), wk, bias, k, s, 1 if full else 0, True)
        _bound(_nchw(out), ref, u, f"dwconv16 C {Cc}")
        assert torch.isfinite(part).all()   # every slot written
        acc = torch.zeros(2, Cc, device=DEV)
        for sp in range(part.shape[1]):     # the SE kernel's order
            acc = acc + part[:, sp]
        _bound(acc / (ref.shape[2] * ref.shape[3]), ref.mean((2, 3)), 0.0, f"pool partials ({part.shape[1]} slots)")
        out2, _ = _dwconv16(mode, _nhwc(x), wk, bias, k, s, 1 if full else 0, False)
        assert torch.equal(out2, out)       # the kernel without the pooling sums stores the same values


@pytest.mark.parametrize("mode", MODES)
def test_dwconv16_empty_pool_slots_add_zero(mode):
    """3 x 2 pixels in a workgroup of 32 pixel lanes: small integers make every sum exact, so the partial is the exact sum only if
    the 26 empty lanes (and the channel groups past C) added exactly 0."""
    dt = DT[mode][0]
    torch.manual_seed(7)
    Cc = 24
    x = torch.randint(-3, 4, (2, Cc, 3, 2), device=DEV).float()
    w = torch.randint(-2, 3, (Cc, 1, 3, 3), device=DEV).float()
    ref = F.conv2d(R._same(x.double(), 3, 1), w.double(), None, 1, 0, 1, Cc)
    out, part = _dwconv16(mode, _nhwc(x.to(dt)), w[:, 0].permute(1, 2, 0).contiguous(), None, 3, 1, 0, True)
    assert torch.equal(_nchw(out).double(), ref)
    assert part.shape[1] == 1
    assert torch.equal(part[:, 0].double(), ref.sum((2, 3)))


def _pack_pw(w, dt):
    """w [co, ci] -> (packed dtype tensor, Kp, Np): [Np / 16][Kp / 32][4 k groups][16 columns][8 k], the layout the header states."""
    co, ci = w.shape
    kp, np_ = -(-ci // 32) * 32, -(-co // 64) * 64
    wp = torch.zeros(np_, kp, device=DEV)
    wp[:co, :ci] = w
    return wp.reshape(np_ // 16, 16, kp // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(dt), kp, np_


def _pointwise16(mode, x, w, bias, act, in_scale=None, residual=None, out=None, img_stride=None, row_stride=None, off=0):
    dt, code, _ = DT[mode]
    B, H, W, ci = x.shape
    co = w.shape[0]
    wp, kp, np_ = _pack_pw(w.float(), dt)
    bp = torch.zeros(np_, device=DEV)
    bp[:co] = bias
    f32 = out is not None
    if out is None:
        out = torch.full((B, H, W, co), float("nan"), device=DEV, dtype=dt)
    p = capi.DetPointwise16(x.data_ptr(), wp.data_ptr(), bp.data_ptr(), None if in_scale is None else in_scale.data_ptr(),
                            None if residual is None else residual.data_ptr(), out.data_ptr(), B * H * W,
                            H * W * co if img_stride is None else img_stride, co if row_stride is None else row_stride, off, H * W,
                            ci, co, kp, np_, act, code, 1 if f32 else 0)
    capi.call("stl_det_pointwise16", C.byref(p), _st())
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci,co", [(8, 8), (40, 24), (1152, 344), (64, 36)])
def test_pointwise16_se_residual(mode, ci, co):
    dt, _, u = DT[mode]
    torch.manual_seed(ci)
    B, H, W = 2, 7, 9
    x = torch.randn(B, H, W, ci, device=DEV).to(dt)
    w = (torch.randn(co, ci, device=DEV) / ci ** 0.5).to(dt)
    bias = torch.randn(co, device=DEV)
    sc = torch.rand(B, ci, device=DEV)
    xs = (x.float() * sc[:, None, None, :]).to(dt)   # the kernel's operand: fp32 product, rounded once
    res = torch.randn(B, H, W, co, device=DEV).to(dt)
    ref = F.silu(xs.double() @ w.double().t() + bias.double()) + res.double()
    _bound(_pointwise16(mode, x, w, bias, 1, sc, res), ref, u, f"pointwise16 {ci} -> {co}")
    if co != 36:
        return
    # a head header: the sigmoid of two levels into one fp32 [B, A, 4] tensor with the heads' image stride, row stride and offset
    k, sentinel = co // 9, -77.0
    x2 = torch.randn(B, 4, 5, ci, device=DEV).to(dt)
    A = (H * W + 4 * 5) * 9 + 5
    out = torch.full((B, A, k), sentinel, device=DEV)
    _pointwise16(mode, x, w, bias, 2, out=out, img_stride=A * k, row_stride=co, off=0)
    _pointwise16(mode, x2, w, bias, 2, out=out, img_stride=A * k, row_stride=co, off=H * W * 9 * k)
    ref = torch.cat([torch.sigmoid(t.double() @ w.double().t() + bias.double()).reshape(B, -1, k) for t in (x, x2)], 1)
    _bound(out[:, :A - 5], ref, 0.0, "pointwise16 heads")
    assert (out[:, A - 5:] == sentinel).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", [(17, 12), (16, 9)])
def test_stem16(mode, hw):
    dt, code, u = DT[mode]
    torch.manual_seed(hw[1])
    B, Co = 2, 40
    x = torch.randn(B, 3, *hw, device=DEV)
    w = torch.randn(Co, 3, 3, 3, device=DEV)
    bias = torch.randn(Co, device=DEV)
    ref = F.silu(F.conv2d(R._same(x.double(), 3, 2), w.double(), bias.double(), 2))
    out = torch.full((B, ref.shape[2], ref.shape[3], Co), float("nan"), device=DEV, dtype=dt)
    xn, wk = _nhwc(x), w.permute(2, 3, 1, 0).contiguous()
    capi.call("stl_det_stem16", code, xn.data_ptr(), wk.data_ptr(), bias.data_ptr(), out.data_ptr(), B, hw[0], hw[1], Co, _st())
    _bound(_nchw(out), ref, u, "stem16")


@pytest.mark.parametrize("mode", MODES)
def test_bifpn_node16_and_zero_padded_pool(mode):
    dt, code, u = DT[mode]
    torch.manual_seed(5)
    B, Cc = 2, 16
    same = torch.randn(B, 8, 8, Cc, device=DEV).to(dt)
    low = torch.randn(B, 4, 4, Cc, device=DEV).to(dt)
    high = (-torch.rand(B, 15, 15, Cc, device=DEV) - 0.1).to(dt)   # all negative: the zero padding decides every border maximum
    wparam = torch.tensor([0.7, -0.2, 1.3], device=DEV)
    f = capi.DetFuse()
    f.B, f.H, f.W, f.C, f.nterms = B, 8, 8, Cc, 3
    f.t[0] = capi.DetTerm(same.data_ptr(), 0, 8, 8, 0)
    f.t[1] = capi.DetTerm(low.data_ptr(), 1, 4, 4, 0)
    f.t[2] = capi.DetTerm(high.data_ptr(), 2, 15, 15, 0)
    f.wparam = wparam.data_ptr()
    out = torch.full((B, 8, 8, Cc), float("nan"), device=DEV, dtype=dt)
    f.out = out.data_ptr()
    capi.call("stl_det_fuse16", C.byref(f), code, _st())
    w = F.relu(wparam)
    w = (w / (w.sum() + 1e-4)).double()
    pooled = R._pool(_nchw(high).double())
    assert (pooled[..., -1, :] == 0).all() and (pooled[..., 0, :] == 0).all()   # border windows reach the zero padding
    ref = F.silu(w[0] * _nchw(same).double() + w[1] * F.interpolate(_nchw(low).double(), scale_factor=2, mode="nearest") + w[2] * pooled)
    _bound(_nchw(out), ref, u, "fuse16")
    # even size: 1 pad after only; a plain pooled map is exact
    g8 = (torch.randn(B, 8, 8, Cc, device=DEV) - 3).to(dt)
    f2 = capi.DetFuse()
    f2.B, f2.H, f2.W, f2.C, f2.nterms = B, 4, 4, Cc, 1
    f2.t[0] = capi.DetTerm(g8.data_ptr(), 2, 8, 8, 0)
    o2 = torch.full((B, 4, 4, Cc), float("nan"), device=DEV, dtype=dt)
    f2.out = o2.data_ptr()
    capi.call("stl_det_fuse16", C.byref(f2), code, _st())
    assert torch.equal(_nchw(o2).float(), R._pool(_nchw(g8).float()))


def test_se16_from_partials():
    torch.manual_seed(3)
    B, HW, nparts, Cc, Cs = 2, 143, 5, 96, 4
    part = torch.randn(B, nparts, Cc, device=DEV) * 30
    w1, b1 = torch.randn(Cs, Cc, device=DEV) / 10, torch.randn(Cs, device=DEV)
    w2, b2 = torch.randn(Cc, Cs, device=DEV), torch.randn(Cc, device=DEV)
    sc = torch.full((B, Cc), float("nan"), device=DEV)
    capi.call("stl_det_se16", part.data_ptr(), B, HW, nparts, Cc, Cs, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
              sc.data_ptr(), _st())
    m = part.double().sum(1) / HW
    ref = torch.sigmoid(F.silu(m @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double())
    _bound(sc, ref, 0.0, "se16")


@pytest.mark.parametrize("mode", MODES)
def test_c_not_multiple_of_8_is_an_error(mode):
    dt, code, _ = DT[mode]
    B, H, W, Cc = 1, 4, 4, 12
    x = torch.zeros(B, H, W, Cc, device=DEV, dtype=dt)
    w = torch.zeros(3, 3, Cc, device=DEV)
    out = torch.full((B, H, W, 16), 5.0, device=DEV, dtype=dt)
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        capi.call("stl_det_dwconv16", code, x.data_ptr(), w.data_ptr(), None, out.data_ptr(), None, B, H, W, Cc, 3, 1, 0, _st())
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        capi.call("stl_det_stem16", code, x.data_ptr(), w.data_ptr(), w.data_ptr(), out.data_ptr(), B, 8, 8, Cc, _st())
    wp = torch.zeros(64 * 32, device=DEV, dtype=dt)
    p = capi.DetPointwise16(x.data_ptr(), wp.data_ptr(), None, None, None, out.data_ptr(), B * H * W, H * W * 16, 16, 0, H * W, Cc, 16, 32,
                            64, 0, code, 0)
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        capi.call("stl_det_pointwise16", C.byref(p), _st())
    f = capi.DetFuse()
    f.B, f.H, f.W, f.C, f.nterms = B, H, W, Cc, 1
    f.t[0] = capi.DetTerm(x.data_ptr(), 0, H, W, 0)
    f.out = out.data_ptr()
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        capi.call("stl_det_fuse16", C.byref(f), code, _st())
    with pytest.raises(RuntimeError, match="dtype"):
        capi.call("stl_det_fuse16", C.byref(f), 0, _st())
    torch.cuda.synchronize()
    assert (out == 5.0).all()


# ------------------------------------------------------------------------------------------------ end to end
def _chw():
    return [im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in R.images()]


@pytest.fixture(scope="module")
def sd0(g):
    return R.synth_state_dict(_layout(g, 0))


@pytest.fixture(scope="module")
def yard0(sd0):
    """The fp32 yardstick Y at D0 on the host (left unchanged by the tests)."""
    with torch.no_grad():
        return R.eager_forward(sd0, 0, 1, R16.canvas())


def _model(sd, name, mode):
    m = E.setup_detector("efficientdet", name, compute_dtype=mode)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def models0(sd0):
    return {mode: _model(sd0, "d0", mode) for mode in MODES}


def _flat(out):
    feats, reg, cls = out[0], out[1], out[2]
    return [("reg", reg), ("cls", cls)] + [(f"f{i}", f) for i, f in enumerate(feats)]


def _against_emulation(dev_out, yard, emu, names):
    bad = []
    for (n, d), (_, y), (_, e) in zip(_flat(dev_out), _flat(yard), _flat(emu)):
        if n not in names:
            continue
        e_dev, e_emu = R16.rel_err(d, y), R16.rel_err(e, y)
        print(f"{n}: e_dev {e_dev:.3e} e_emu {e_emu:.3e} ratio {e_dev / e_emu:.2f}")
        if not e_dev <= 2 * e_emu:
            bad.append((n, e_dev, e_emu))
    assert not bad, bad


ALL = ("reg", "cls", "f0", "f1", "f2", "f3", "f4")


@pytest.mark.parametrize("mode", MODES)
def test_d0_error_within_twice_the_emulation(mode, sd0, yard0, models0):
    """e_dev(t) = max|device16 - Y| / max|Y| <= 2 e_emu(t) for reg, cls and the five features; Y the fp32 yardstick
    detector_ref.eager_forward, e_emu the same figure of the storage-rounding emulation detector16_ref.forward16."""
    dt = DT[mode][0]
    m = models0[mode]
    out = m(_chw(), postprocess=False)
    with torch.no_grad():
        emu = R16.forward16(sd0, 0, 1, R16.canvas(), R16.rounder(dt), dt)
    p = m._plans[2]
    assert all(f.dtype == dt for f, _ in p.feats) and all(t.dtype == dt for t in p.backbone)
    assert all(t.dtype == dt for t in p._keep if torch.is_tensor(t) and t.dim() == 4 and t is not p.canvas)
    assert p.canvas.dtype == p.reg.dtype == p.cls.dtype == torch.float32
    names = {name for _, name, _ in p.calls}
    assert names == {"stl_det_stem16", "stl_det_dwconv16", "stl_det_se16", "stl_det_pointwise16", "stl_det_fuse16"}
    assert all(t.dtype == torch.float32 for t in out[0]) and out[1].dtype == out[2].dtype == torch.float32
    assert [tuple(t.shape) for t in out[0]] == [tuple(t.shape) for t in yard0[0]]
    fp32 = _model(sd0, "d0", "fp32")
    reg32 = fp32(_chw(), postprocess=False)[1]
    assert not torch.equal(reg32, out[1])   # the 16-bit path ran
    assert len(fp32._plans[2].calls) == len(p.calls) and fp32._plans[2].launches - p.launches == len(E.block_specs(0))
    assert p.bytes < 0.6 * fp32._plans[2].bytes
    _against_emulation(out, yard0, emu, ALL)


@pytest.mark.parametrize("mode", MODES)
def test_d0_detections_from_own_heads(mode, models0):
    m = models0[mode]
    _, reg, cls, _ = m(_chw(), postprocess=False)
    dets = m(_chw())
    own = R.postprocess(E.anchors(0), reg.cpu().numpy(), cls.cpu().numpy(), 0.5, 0.5)
    metas = [E.resize_meta(*im.shape[:2]) for im in R.images()]
    for i, d in enumerate(dets):
        ob, oc, os_ = own[i]
        assert len(os_) > 0
        np.testing.assert_array_equal(d["scores"].numpy(), os_)
        np.testing.assert_array_equal(d["labels"].numpy(), oc + 1)
        np.testing.assert_allclose(d["boxes"].numpy(), E.invert_affine(metas[i], ob), rtol=0, atol=1e-3)


@pytest.mark.parametrize("mode", MODES)
def test_bitwise_repeatable16(mode, models0):
    m = models0[mode]
    a = [t.clone() for t in m(_chw(), postprocess=False)[1:3]]
    b = [t.clone() for t in m(_chw(), postprocess=False)[1:3]]
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("mode", MODES)
def test_d3_error_within_twice_the_emulation(mode, g):
    dt = DT[mode][0]
    sd = R.synth_state_dict(_layout(g, 3))
    x = R16.canvas()[:1]
    with torch.no_grad():
        yard = R.eager_forward(sd, 3, 1, x)
        emu = R16.forward16(sd, 3, 1, x, R16.rounder(dt), dt)
    out = _model(sd, "d3", mode)(_chw()[:1], postprocess=False)
    _against_emulation(out, yard, emu, ("reg", "cls"))


def test_f16_range_guard(sd0):
    """The stem's BN scale times 1e6: the activations overflow f16 to inf (arithmetic, no device fault) and the forward raises;
    bf16 has fp32's range and returns finite outputs."""
    sd = dict(sd0)
    sd["backbone_net.model._bn0.weight"] = sd["backbone_net.model._bn0.weight"] * 1e6
    with pytest.raises(FloatingPointError, match="bf16"):
        _model(sd, "d0", "f16")(_chw()[:1], postprocess=False)
    _, reg, cls, _ = _model(sd, "d0", "bf16")(_chw()[:1], postprocess=False)
    assert torch.isfinite(reg).all() and torch.isfinite(cls).all()


def test_fp32_plan_undisturbed(g, sd0, models0):
    for mode in MODES:
        models0[mode](_chw(), postprocess=False)
    m = _model(sd0, "d0", "fp32")
    cls = m(_chw(), postprocess=False)[2]
    assert m._plans[2].reg.dtype == torch.float32 and all(f.dtype == torch.float32 for f, _ in m._plans[2].feats)
    a, b = cls.float().cpu(), torch.as_tensor(g["cls"]).float()
    err = (a - b).abs().max().item()
    assert err <= 1e-3 * b.abs().max().item(), err
