"""GPU: fine-tuning the EfficientDet heads in 16 bit (compute_dtype="f16": f16 forward tensors, bf16 gradients in flight, fp32 sums
and fp32 weight gradients; csrc/detector_train.hip, stlpose_amd/detector_train.py).

Kernels.  Inputs are drawn exactly representable in the types the kernels read them in (x both f16 and bf16, dy bf16, the transposed
pack bf16), so every product is exact in fp32 and the fp64 result on those values is the truth Y.  The fp32 outputs (dw, db) are held
to the fp32 file's rule max(8 e32, 1e-6), e32 the error of the fp32 torch evaluation of the same values; a bf16 output (dx) is held
elementwise to |dx - Y| <= 2^-8 |Y| + 8 e32 max|Y|: one bf16 rounding plus the accumulation-order allowance.

The whole method.  Each loss and each head gradient G has e = max|G - Y64| / max|Y64| against the fp64 yardstick
tests/detector_train_ref.py run from the features the GPU made, and is held to max(2 e16, 2^-9): e16 is the same figure of the
storage-rounding emulation tests/detector_train16_ref.py (factor 2 as tests/test_detector16_gpu.py allows its forward), and 2^-9 is
half a bf16 unit at the tensor's largest element.  Every e, e16 and ratio is printed (run with -s).  Measured on an MI355X:
  D0  gradients e 0 .. 7.7e-3, e16 0 .. 7.9e-3, e / e16 0.76 .. 1.19 (the 18 regressor BN gradients of the three levels without a
      positive anchor are exactly zero in the device's result, the yardstick and the emulation); classification loss e 6.5e-6
      (e16 6.7e-6, 0.97); regression loss e 1.7e-5 (e16 1.8e-6, 9.2: held by the floor, which it is a hundred times under)
  D3  gradients e 1.1e-3 .. 1.4e-2, e16 9.2e-4 .. 1.0e-2, e / e16 0.50 .. 1.71; losses e 2.0e-6 and 2.6e-5 (1.03 and 1.23)"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, efficientdet as E
from tests import detector_ref as R, detector_train16_ref as TR16, detector_train_ref as TR
from tests.test_detector_train_gpu import CLS_HEADER_BIAS, CLS_HEADER_SCALE, MARGIN, TARGETS, _check_yardstick, _hold

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = 2, 1        # STL_F16, STL_BF16
TORCH16 = {F16: torch.float16, BF16: torch.bfloat16}
U_BF16 = 2.0 ** -8      # unit roundoff of bf16
FLOOR16 = 2.0 ** -9


def _st():
    return torch.cuda.current_stream().cuda_stream


def _both16(t):
    """randn values representable in bf16 and in f16 at once (bf16's 8 significant bits, inside f16's normal range)."""
    t = t.to(torch.bfloat16).float()
    t[t.abs() < 2.0 ** -10] = 0
    assert torch.equal(t.half().float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)
    return t


def _hold_bf16(name, got, y64, y32):
    """A bf16 output, elementwise: |got - Y| <= 2^-8 |Y| + MARGIN e32 max|Y|."""
    got, y64 = got.double().cpu(), y64.double().cpu()
    assert got.shape == y64.shape and torch.isfinite(got).all(), name   # a NaN is an element the kernel did not write
    e32, mx = TR.rel_err(y32, y64), y64.abs().max().item()
    excess = ((got - y64).abs() - (U_BF16 * y64.abs() + MARGIN * e32 * mx)).max().item()
    print(f"{name}: max|err| {(got - y64).abs().max().item():.3e} max|Y| {mx:.3e} e32 {e32:.3e} worst excess over the bound {excess:.3e}")
    assert excess <= 0, (name, excess, mx)


# ------------------------------------------------------------------------------------------------ pointwise backward
@pytest.mark.parametrize("xdtype", [F16, BF16])
@pytest.mark.parametrize("M", [16, 70, 4100])
@pytest.mark.parametrize("ci,co", [(64, 64), (160, 160), (64, 9), (160, 36)])
def test_pointwise16_backward(M, ci, co, xdtype):
    """dX = dY W'^T (bf16 out), dW' = X^T dY, db' = sum dY (fp32 out).  Co 9 / 36 are the headers: dY is fp32, read out of a
    [B, A, k] tensor at a non-zero anchor offset.  M = 16 is below one 32-deep MFMA step of the weight gradient, 70 a multiple of
    neither 32 nor 64, 4100 more than one slab.  x is stored as f16 (what a model trains with) or as bf16: the same values, so the
    same results."""
    g = torch.Generator().manual_seed(M + ci + co)
    B, hw = 2, M // 2
    x = _both16(torch.randn(M, ci, generator=g))
    w = (torch.randn(co, ci, generator=g) / ci ** 0.5).to(torch.bfloat16).float()
    header = co in (9, 36)
    if header:
        k, lead = co // 9, 7
        A = lead + hw * 9 + 5
        full = torch.randn(B, A, k, generator=g).to(torch.bfloat16).float()   # fp32 storage, bf16-representable values
        dy = full[:, lead:lead + hw * 9].reshape(M, co)
        strides = (A * k, co, lead * k)
    else:
        full = torch.randn(M, co, generator=g).to(torch.bfloat16).float()
        dy, strides = full, (hw * co, co, 0)
    wt, kt, nt = E.pack_transposed(w.double())
    assert torch.equal(E.unpack_transposed(wt, ci, co).float(), w.t())
    dx64, dw64, db64 = dy.double() @ w.double(), x.double().t() @ dy.double(), dy.double().sum(0)
    dx32, dw32, db32 = dy @ w, x.t() @ dy, dy.sum(0)
    slabs = capi.lib().stl_det_pointwise16_bwd_slabs(M)
    if M == 4100:
        assert slabs > 1

    def run():
        xd, wd, fd = x.to(TORCH16[xdtype]).to(DEV), wt.to(DEV), (full if header else full.to(torch.bfloat16)).to(DEV)
        dx = torch.full((M, ci), float("nan"), device=DEV, dtype=torch.bfloat16)
        dw, db = torch.full((ci, co), float("nan"), device=DEV), torch.full((co,), float("nan"), device=DEV)
        part = torch.empty(slabs * (ci * co + co), device=DEV)
        p = capi.DetPointwise16Bwd(xd.data_ptr(), wd.data_ptr(), fd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), part.data_ptr(),
                                   M, strides[0], strides[1], strides[2], hw, ci, co, kt, nt, xdtype, 1 if header else 0, 0)
        capi.call("stl_det_pointwise16_bwd_data", C.byref(p), _st())
        capi.call("stl_det_pointwise16_bwd_weight", C.byref(p), _st())
        torch.cuda.synchronize()
        return dx.cpu(), dw.cpu(), db.cpu()
    got = run()
    tag = f"pointwise16_bwd M={M} {ci}->{co} x {TORCH16[xdtype]}"
    _hold_bf16(f"{tag} dx", got[0], dx64, dx32)
    _hold(f"{tag} dw", got[1], dw64, dw32)
    _hold(f"{tag} db", got[2], db64, db32)
    assert all(torch.equal(a, b) for a, b in zip(run(), got))


def test_pointwise16_backward_checks_its_arguments():
    M, ci, co = 16, 64, 64
    x = torch.zeros(M + 1, ci, device=DEV, dtype=torch.float16)
    dy = torch.zeros(M + 1, co, device=DEV, dtype=torch.bfloat16)
    wt = torch.zeros(64 * 64, device=DEV, dtype=torch.bfloat16)
    dx = torch.full((M, ci), 5.0, device=DEV, dtype=torch.bfloat16)
    dw, db, part = torch.full((ci, co), 5.0, device=DEV), torch.full((co,), 5.0, device=DEV), torch.empty(ci * co + co, device=DEV)

    def desc(**kw):
        f = dict(x=x.data_ptr(), wt=wt.data_ptr(), dy=dy.data_ptr(), dx=dx.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(),
                 partial=part.data_ptr(), M=M, dy_img_stride=M * co, dy_row_stride=co, dy_off=0, HW=M, Ci=ci, Co=co, Kp=64, Np=64,
                 xdtype=F16, dy_f32=0, pad_=0)
        f.update(kw)
        return capi.DetPointwise16Bwd(**f)
    for name, match, p in (("stl_det_pointwise16_bwd_weight", "dtype", desc(xdtype=0)),
                           ("stl_det_pointwise16_bwd_weight", "null", desc(x=None)),
                           ("stl_det_pointwise16_bwd_weight", "aligned", desc(x=x.data_ptr() + 2)),
                           ("stl_det_pointwise16_bwd_weight", "C % 8 == 0", desc(Ci=60)),
                           ("stl_det_pointwise16_bwd_data", "null", desc(wt=None)),
                           ("stl_det_pointwise16_bwd_data", "aligned", desc(dy=dy.data_ptr() + 2)),
                           ("stl_det_pointwise16_bwd_data", "multiples of 8", desc(dy_off=4)),
                           ("stl_det_pointwise16_bwd_data", "transposed pack", desc(Kp=48))):
        with pytest.raises(RuntimeError, match=match):
            capi.call(name, C.byref(p), _st())
    torch.cuda.synchronize()
    assert (dx == 5.0).all() and (dw == 5.0).all() and (db == 5.0).all()   # nothing was launched


# ------------------------------------------------------------------------------------------------ depthwise backward
@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("c", [64, 160])
@pytest.mark.parametrize("bhw", [(2, 4, 4), (1, 9, 6), (1, 64, 64)])
def test_depthwise16_backward(bhw, c, fused, dtype):
    """y = dwconv3x3_same(x), x = round(swish(z)), x and z stored in dtype (f16 is what a model trains with): dx (bf16) is dL/dx, times swish'(z) from the stored f16 z when fused; dw
    (fp32) sums batch and pixels of x (dtype) dy (bf16), products exact in fp32 (64 x 64: more than one partial sum)."""
    B, H, W = bhw
    g = torch.Generator().manual_seed(B * H + W + c)
    z = torch.randn(B, c, H, W, generator=g).to(TORCH16[dtype])
    w = torch.randn(c, 1, 3, 3, generator=g) / 3
    dy = torch.randn(B, c, H, W, generator=g).to(torch.bfloat16)
    x = F.silu(z.float()).to(TORCH16[dtype])

    def yard(dt):
        xx, ww = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        (F.conv2d(R._same(xx, 3, 1), ww, None, 1, 0, 1, c) * dy.to(dt)).sum().backward()
        gx = xx.grad
        if fused:
            zz = z.to(dt).requires_grad_(True)
            (gx,) = torch.autograd.grad(F.silu(zz), zz, gx)
        return gx.permute(0, 2, 3, 1), ww.grad[:, 0].permute(1, 2, 0)
    dx64, dw64 = yard(torch.float64)
    dx32, dw32 = yard(torch.float32)
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
    zd, dyd, xd, wd = nhwc(z), nhwc(dy), nhwc(x), w[:, 0].permute(1, 2, 0).contiguous().to(DEV)
    parts = capi.lib().stl_det_dwconv16_bwd_parts(B * H * W)
    if H == 64:
        assert parts > 1

    def run():
        dx, dw = torch.full((B, H, W, c), float("nan"), device=DEV, dtype=torch.bfloat16), torch.full((3, 3, c), float("nan"), device=DEV)
        part = torch.empty(parts * 9 * c, device=DEV)
        capi.call("stl_det_dwconv16_bwd_data", dyd.data_ptr(), wd.data_ptr(), zd.data_ptr() if fused else None, dx.data_ptr(), B, H, W, c,
                  dtype, _st())
        capi.call("stl_det_dwconv16_bwd_weight", dtype, xd.data_ptr(), dyd.data_ptr(), part.data_ptr(), dw.data_ptr(), B, H, W, c, _st())
        torch.cuda.synchronize()
        return dx.cpu(), dw.cpu()
    got = run()
    _hold_bf16(f"dwconv16_bwd {bhw} C={c} fused={fused} {TORCH16[dtype]} dx", got[0], dx64, dx32)
    _hold(f"dwconv16_bwd {bhw} C={c} fused={fused} {TORCH16[dtype]} dw", got[1], dw64, dw32)
    assert all(torch.equal(a, b) for a, b in zip(run(), got))


def test_depthwise16_backward_checks_its_arguments():
    B, H, W, c = 1, 4, 4, 12
    t16 = torch.zeros(B, H, W, 16, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(3, 3, 16, device=DEV)
    dx, dw = torch.full((B, H, W, 16), 5.0, device=DEV, dtype=torch.bfloat16), torch.full((3, 3, 16), 5.0, device=DEV)
    part = torch.empty(9 * 16, device=DEV)
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        capi.call("stl_det_dwconv16_bwd_data", t16.data_ptr(), w.data_ptr(), None, dx.data_ptr(), B, H, W, c, F16, _st())
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        capi.call("stl_det_dwconv16_bwd_weight", F16, t16.data_ptr(), t16.data_ptr(), part.data_ptr(), dw.data_ptr(), B, H, W, c, _st())
    with pytest.raises(RuntimeError, match="dtype"):
        capi.call("stl_det_dwconv16_bwd_weight", 0, t16.data_ptr(), t16.data_ptr(), part.data_ptr(), dw.data_ptr(), B, H, W, 16, _st())
    with pytest.raises(RuntimeError, match="dtype"):
        capi.call("stl_det_dwconv16_bwd_data", t16.data_ptr(), w.data_ptr(), t16.data_ptr(), dx.data_ptr(), B, H, W, 16, 0, _st())
    with pytest.raises(RuntimeError, match="null"):
        capi.call("stl_det_dwconv16_bwd_data", None, w.data_ptr(), None, dx.data_ptr(), B, H, W, 16, F16, _st())
    with pytest.raises(RuntimeError, match="aligned"):
        capi.call("stl_det_dwconv16_bwd_data", t16.data_ptr() + 2, w.data_ptr(), None, dx.data_ptr(), B, H, W, 16, F16, _st())
    torch.cuda.synchronize()
    assert (dx == 5.0).all() and (dw == 5.0).all()


# ------------------------------------------------------------------------------------------------ the training forward's pointwise
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_pointwise16_train_keeps_z_and_equals_the_inference_launch(dtype):
    """out equals stl_det_pointwise16's bit for bit; z equals, bit for bit, the fp32 pre-activation (the same launch with act 0 and an
    fp32 output) rounded once to dtype."""
    M, ci, co = 70, 64, 64
    dt = TORCH16[dtype]
    g = torch.Generator().manual_seed(70)
    x = torch.randn(M, ci, generator=g).to(dt)
    w = (torch.randn(co, ci, generator=g) / ci ** 0.5).to(dt)
    bias = torch.randn(co, generator=g)
    wp = torch.zeros(64, 64)
    wp[:co, :ci] = w.float()
    wp = wp.reshape(4, 16, 2, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(dt).to(DEV)
    xd, bd = x.to(DEV), bias.to(DEV)
    outs = [torch.full((M, co), float("nan"), device=DEV, dtype=dt) for _ in range(3)]
    z32 = torch.full((M, co), float("nan"), device=DEV)

    def desc(out, act=1, out_f32=0):
        return capi.DetPointwise16(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), None, None, out.data_ptr(), M, M * co, co, 0, M, ci, co, 64,
                                   64, act, dtype, out_f32)
    capi.call("stl_det_pointwise16", C.byref(desc(outs[0])), _st())
    capi.call("stl_det_pointwise16_train", C.byref(desc(outs[1])), outs[2].data_ptr(), _st())
    capi.call("stl_det_pointwise16", C.byref(desc(z32, act=0, out_f32=1)), _st())
    torch.cuda.synchronize()
    assert torch.isfinite(z32).all() and torch.equal(outs[2], z32.to(dt))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    z64 = x.double() @ w.double().t() + bias.double()
    err = (outs[2].double().cpu() - z64).abs() - (2.0 ** (-11 if dtype == F16 else -8) * z64.abs() + 1e-5 * z64.abs().max())   # one rounding of the fp32 sum
    print(f"pointwise16_train z: worst excess over the bound {err.max().item():.3e}")
    assert torch.isfinite(outs[2]).all() and err.max().item() <= 0
    p = desc(outs[1])
    p.act = 0
    with pytest.raises(RuntimeError, match="swish"):
        capi.call("stl_det_pointwise16_train", C.byref(p), outs[2].data_ptr(), _st())
    with pytest.raises(RuntimeError, match="null"):
        capi.call("stl_det_pointwise16_train", C.byref(desc(outs[1])), None, _st())


# ------------------------------------------------------------------------------------------------ the whole method
def _model(cc, mode="f16", sd=None):
    m = E.setup_detector("efficientdet", "d3" if cc else "d0", compute_dtype=mode)
    if sd is None:
        sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        sd["classifier.header.pointwise_conv.conv.weight"] = sd["classifier.header.pointwise_conv.conv.weight"] * CLS_HEADER_SCALE
        sd["classifier.header.pointwise_conv.conv.bias"] = torch.full_like(sd["classifier.header.pointwise_conv.conv.bias"], CLS_HEADER_BIAS)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd


def _chw(n):
    return [torch.from_numpy(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255)) for im in R.images()[:n]]


def _step(m, chw, targets):
    """detection_loss + backward on clean .grad -> ({loss}, {head parameter: grad})"""
    m.zero_grad(set_to_none=True)
    loss = m.detection_loss(chw, targets)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in loss.items()},
            {k: p.grad.clone() for k, p in m.named_parameters() if k.startswith(("regressor.", "classifier."))})


def _run(cc):
    """One f16 detection_loss + backward; the fp64 yardstick and the storage-rounding emulation run from the features the GPU made."""
    from stlpose_amd import detector_train as T
    m, sd = _model(cc)
    targets = TARGETS[cc]
    chw = _chw(len(targets))
    o = dict(m=m, sd=sd, chw=chw, targets=targets)
    with torch.no_grad():
        feats, o["reg_inf"], o["cls_inf"], _ = m(chw, postprocess=False)
    o["buffers"] = {k: v.clone() for k, v in m.named_buffers()}
    o["plan"] = m.plan(len(chw), DEV)
    m.train()   # detection_loss works whatever .training is; BN stays frozen
    loss = m.detection_loss(chw, targets)
    o["loss"] = loss
    tr = o["plan"].train
    o["tr"] = tr
    o["reg_train"], o["cls_train"], o["npos"] = tr.reg.clone(), tr.cls.clone(), tr.npos.cpu().tolist()
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    m.eval()
    gt, offsets = T.pack_targets(targets, [tuple(c.shape[1:]) for c in chw], 1)
    args = (sd, cc, 1, feats, torch.from_numpy(m.anchors_np), torch.from_numpy(gt), offsets.tolist())
    o["y64"] = TR.method_yardstick(*args, torch.float64)
    o["emu"] = TR16.method_yardstick(*args, torch.float64, TR16.device_stores())
    return o


@pytest.fixture(scope="module")
def d0():
    return _run(0)


def _check_grads16(o, tag):
    m, (c64, r64, g64, *_), (c16, r16, g16, *_) = o["m"], o["y64"], o["emu"]
    named = dict(m.named_parameters())
    assert set(g64) == {k for k in named if k.startswith(("regressor.", "classifier."))}
    rows = [("classification", o["loss"]["classification"], c64, c16), ("regression", o["loss"]["regression"], r64, r16)]
    for k in sorted(g64):
        assert named[k].grad is not None and named[k].grad.shape == named[k].shape and named[k].grad.dtype == torch.float32, k
        rows.append((k, named[k].grad, g64[k], g16[k]))
    bad, ratios = [], []
    for name, got, y, emu in rows:
        e, e16 = TR.rel_err(got, y), TR.rel_err(emu, y)
        ratios.append(e / e16 if e16 else float("inf"))
        print(f"{tag} {name}: e {e:.3e} e16 {e16:.3e} ratio {ratios[-1]:.2f}")
        if not e <= max(2 * e16, FLOOR16):
            bad.append((name, e, e16))
    print(f"{tag}: e / e16 from {min(ratios):.2f} to {max(ratios):.2f}")
    assert not bad, bad


def test_training_forward_equals_f16_inference_bit_for_bit(d0):
    assert torch.equal(d0["reg_train"], d0["reg_inf"]) and torch.equal(d0["cls_train"], d0["cls_inf"])
    assert all(t.dtype == torch.float32 and t.dim() == 0 and t.is_cuda for t in d0["loss"].values())
    tr = d0["tr"]
    assert tr.ga.dtype == tr.gb.dtype == torch.bfloat16
    assert {n for _, n, _ in tr.fwd} == {"stl_det_dwconv16", "stl_det_pointwise16", "stl_det_pointwise16_train"}
    assert {n for _, n, _ in tr.bwd} == {"stl_det_pointwise16_bwd_weight", "stl_det_pointwise16_bwd_data", "stl_det_dwconv16_bwd_weight",
                                         "stl_det_dwconv16_bwd_data"}
    assert all(t.dtype == torch.float16 for t in tr.fwd.keep if torch.is_tensor(t) and t.dim() == 4 and t.shape[-1] == 64)


def test_losses_and_head_gradients_within_twice_the_emulation(d0):
    _check_yardstick(d0)
    assert d0["npos"] == d0["y64"][5]
    _check_grads16(d0, "d0/f16")


def test_trunk_is_frozen_and_buffers_untouched(d0):
    m = d0["m"]
    for k, p in m.named_parameters():
        if not k.startswith(("regressor.", "classifier.")):
            assert p.grad is None, k
    for k, v in m.named_buffers():
        assert torch.equal(v, d0["buffers"][k]), k


def test_two_runs_are_bitwise_equal(d0):
    a = _step(d0["m"], d0["chw"], d0["targets"])
    b = _step(d0["m"], d0["chw"], d0["targets"])
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_stale_forward_raises(d0):
    m = d0["m"]
    first = m.detection_loss(d0["chw"], d0["targets"])
    m.detection_loss(d0["chw"], d0["targets"])
    with pytest.raises(RuntimeError, match="stale forward"):
        first["classification"].backward()


def test_sgd_step_keeps_the_plan_and_refolds_both_packs_exactly(d0):
    m = d0["m"]
    _step(m, d0["chw"], d0["targets"])
    heads = [p for k, p in m.named_parameters() if k.startswith(("regressor.", "classifier."))]
    bufs = (m._wbuf, m._wbuf16, m._wbufT16)
    before = m._wbufT16.clone()
    torch.optim.SGD(heads, lr=1e-3).step()
    got = _step(m, d0["chw"], d0["targets"])
    assert m.plan(len(d0["chw"]), DEV) is d0["plan"] and d0["plan"].train is d0["tr"]
    assert all(a is b for a, b in zip(bufs, (m._wbuf, m._wbuf16, m._wbufT16)))
    assert not torch.equal(m._wbufT16, before)   # the step moved the transposed packs
    fresh, _ = _model(0, sd=m.state_dict())
    want = _step(fresh, d0["chw"], d0["targets"])
    assert torch.equal(m._wbuf, fresh._wbuf) and torch.equal(m._wbuf16, fresh._wbuf16) and torch.equal(m._wbufT16, fresh._wbufT16)
    assert all(torch.equal(got[0][k], want[0][k]) for k in want[0])
    assert set(got[1]) == set(want[1]) and all(torch.equal(got[1][k], want[1][k]) for k in want[1])


def test_fp32_model_beside_an_f16_one_is_untouched():
    chw, targets = _chw(2), TARGETS[0]
    alone, sd = _model(0, "fp32")
    want = _step(alone, chw, targets)
    half, _ = _model(0, "f16", sd)
    _step(half, chw, targets)
    beside, _ = _model(0, "fp32", sd)
    got, again = _step(beside, chw, targets), _step(alone, chw, targets)
    assert beside._wbufT16 is None and beside._wbuf16 is None
    assert {n for _, n, _ in beside.plan(2, DEV).train.bwd} == {"stl_det_pointwise_bwd_weight", "stl_det_pointwise_bwd_data",
                                                               "stl_det_dwconv_bwd_weight", "stl_det_dwconv_bwd_data"}
    for other in (got, again):
        assert all(torch.equal(other[0][k], want[0][k]) for k in want[0]) and all(torch.equal(other[1][k], want[1][k]) for k in want[1])


def test_bf16_still_does_not_train():
    m, _ = _model(0, "bf16")
    with pytest.raises(NotImplementedError, match=r"fp32.*f16"):
        m.detection_loss(_chw(1), TARGETS[0][:1])


def test_non_finite_training_forward_raises():
    """The stem's BN scale times 1e6 takes the f16 activations to inf (arithmetic, no device fault): the training forward raises and
    points to fp32."""
    m, sd = _model(0)
    sd = dict(sd)
    sd["backbone_net.model._bn0.weight"] = sd["backbone_net.model._bn0.weight"] * 1e6
    m, _ = _model(0, sd=sd)
    with pytest.raises(FloatingPointError, match='compute_dtype="fp32"'):
        m.detection_loss(_chw(1), TARGETS[0][:1])


def test_d3_gradients_within_twice_the_emulation():
    """C = 160 is no multiple of the 64-wide tiles; five boxes meet the anchors of all five levels."""
    o = _run(3)
    _check_yardstick(o)
    assert o["npos"] == o["y64"][5]
    assert all(g.abs().max() > 0 for k, g in o["y64"][2].items() if k.startswith("regressor.bn_list")), "a level without positives"
    named = dict(o["m"].named_parameters())
    assert all(named[k].grad.abs().max() > 0 for k in o["y64"][2] if k.startswith("regressor.bn_list"))
    _check_grads16(o, "d3/f16")
