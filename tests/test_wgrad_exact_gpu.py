"""GPU: the weight-gradient kernels (wgrad.hip) and the stride-2 data gradient (zero-stuffed source) against fp64 CPU references.

Exact tests: every operand is an integer from {-3..3} without 0, so every product and every fp32 partial sum (< 2^24) is exact in
any order and type; the summed slabs must EQUAL the fp64 reference.  A missed, doubled or misplaced pixel, tap, channel, tile or
split is a non-zero integer.  Transformed sources (BatchNorm on load, BatchNorm backward on load) are held to an elementwise bound
computed from the reference side alone (tests/wgrad_ref.py: bound).  Every case names the kernel instantiation it expects.
All tensors the kernels touch lie between NaN guard bands, so that a stray read shows up as NaN and a stray write in the band."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from stlpose_amd import capi  # noqa: E402
from tests import wgrad_ref as R  # noqa: E402
from tests.gpu_guard import Guarded, launch  # noqa: E402

CODE = {"f32": capi.F32, "bf16": capi.BF16, "f16": capi.F16}
RATIOS = {}         # observed max |err| / E per type (information only: printed, never asserted against)


@functools.lru_cache(maxsize=None)
def exact_device(geom, Ci, Co, T, TY):
    """The integer problem on the device: h as TY, g as T, and an all-NaN tensor for g.y (a PLAIN gradient never reads it)."""
    h, g, ref = R.exact_problem(geom, Ci, Co)
    return Guarded(h.numel(), R.TORCH_DT[TY], h), Guarded(g.numel(), R.TORCH_DT[T], g), Guarded(g.numel(), R.TORCH_DT[TY]), ref


def wgrad_params(row, dt, Ci, Co, nsplit):
    geom, TH, TW = row[:3]
    B, Hi, Wi, ks, s = R.GEOMS[geom]
    Ho, Wo = R.out_hw(geom)
    T, TY = R.TYPES[dt]
    wg = capi.Wgrad()
    wg.dtype, wg.B, wg.Hi, wg.Wi, wg.Ci, wg.Ho, wg.Wo, wg.Co = CODE[T], B, Hi, Wi, Ci, Ho, Wo, Co
    wg.ks, wg.stride, wg.TH, wg.TW, wg.nsplit = ks, s, TH, TW, nsplit
    wg.ydtype = CODE[TY] if TY != T else 0
    return wg


def run_wgrad(wg, expect, inputs):
    """One launch into a NaN slab between guard bands; returns the fp64 sum of the nsplit slabs [Co][tap][Ci] (CPU)."""
    taps = wg.ks * wg.ks
    part = Guarded(wg.nsplit * wg.Co * taps * wg.Ci, torch.float32)
    wg.partial = part.ptr()
    rc, err = launch("stl_conv_wgrad", wg)
    assert rc == 0, err
    name = capi.lib().stl_last_kernel().decode()
    assert R.parse_kernel_name(name) == expect, f"launched {name}, the case expects {expect}"
    assert not torch.isnan(part.t).any(), "slab elements not written, or NaN read from a guard band"
    assert part.bands_intact(), "write outside the slabs"
    for t in inputs:
        assert t.bands_intact()
    return part.t.view(wg.nsplit, wg.Co, taps, wg.Ci).double().sum(0).cpu()


def grid_orders(expect, Ci, Co):
    ch = expect[7]
    return ("1", "0") if -(-Ci // ch) * -(-Co // ch) > 1 else ("1",)   # STL_WGRAD_XCD: XCD-aware 1-D grid / plain 3-D grid


@pytest.mark.parametrize("case", R.exact_cases(), ids=R.case_id)
def test_wgrad_equals_fp64_exactly(case, monkeypatch):
    row, dt, Ci, Co, nsplit = case
    T, TY = R.TYPES[dt]
    expect = R.stated_instantiation(row, dt, Ci, Co, 0)
    h, g, gy, ref = exact_device(row[0], Ci, Co, T, TY)
    for xcd in grid_orders(expect, Ci, Co):
        monkeypatch.setenv("STL_WGRAD_XCD", xcd)
        wg = wgrad_params(row, dt, Ci, Co, nsplit)
        wg.h.x, wg.h.mode = h.ptr(), capi.SRC_PLAIN
        wg.g.x, wg.g.y, wg.g.mode = g.ptr(), gy.ptr(), capi.SRC_PLAIN
        dw = run_wgrad(wg, expect, (h, g, gy))
        bad = (dw != ref).nonzero()
        assert torch.equal(dw, ref), f"XCD={xcd}: {len(bad)} of {ref.numel()} elements differ, first (co, tap, ci) = {bad[0].tolist()}: " \
                                     f"{float(dw[tuple(bad[0])])} != {float(ref[tuple(bad[0])])}"


@pytest.mark.parametrize("case", R.refused_cases(), ids=R.case_id)
def test_wgrad_refuses_a_halo_too_large(case):
    """A tile whose halo no instantiation can stage is refused on the host: an error, and nothing is launched."""
    row, dt, Ci, Co = case
    T, TY = R.TYPES[dt]
    assert R.stated_instantiation(row, dt, Ci, Co, 0) is None
    h, g, gy, _ = exact_device(row[0], Ci, Co, T, TY)
    wg = wgrad_params(row, dt, Ci, Co, 1)
    wg.h.x, wg.h.mode = h.ptr(), capi.SRC_PLAIN
    wg.g.x, wg.g.y, wg.g.mode = g.ptr(), gy.ptr(), capi.SRC_PLAIN
    part = Guarded(Co * wg.ks * wg.ks * Ci, torch.float32)
    wg.partial = part.ptr()
    rc, err = launch("stl_conv_wgrad", wg)
    assert rc != 0 and "halo" in err and "too large" in err, err
    assert torch.isnan(part.t).all()


# ------------------------------------------------------------------------------------------------ transformed sources
def dev(t, keep, dtype=None):
    d = t.to(dtype or t.dtype).contiguous().cuda()
    keep.append(d)
    return d


def shard0(st, keep):
    """[2][C] fp64 sums -> [NSHARD][2][C] with everything in shard 0, as the existing tests build them."""
    out = torch.zeros(capi.NSHARD, 2, st.shape[1], dtype=torch.float64)
    out[0] = st
    return dev(out, keep)


@functools.lru_cache(maxsize=None)
def xform_device(geom, Ci, Co, dt):
    P = R.xform_problem(geom, Ci, Co, dt)
    T, TY = R.TYPES[dt]
    return (Guarded(P["x"].numel(), R.TORCH_DT[TY], P["x"]), Guarded(P["dy"].numel(), R.TORCH_DT[T], P["dy"]),
            Guarded(P["y"].numel(), R.TORCH_DT[TY], P["y"]))


@pytest.mark.parametrize("case", R.xform_cases(), ids=R.case_id)
def test_wgrad_transformed_sources_within_fp64_bound(case):
    """h as BatchNorm (batch statistics, with and without ReLU; eval mode) or PLAIN, g as BatchNorm backward or PLAIN:
    |got - ref| <= E elementwise, ref and E from the stored tensors in fp64 (tests/wgrad_ref.py)."""
    row, dt, Ci, Co, nsplit, hmode, gmode = case
    geom = row[0]
    B, Hi, Wi, ks, s = R.GEOMS[geom]
    Ho, Wo = R.out_hw(geom)
    P = R.xform_problem(geom, Ci, Co, dt)
    ref, E = R.xform_reference(geom, Ci, Co, dt, hmode, gmode)
    x, dy, y = xform_device(geom, Ci, Co, dt)
    keep = []
    wg = wgrad_params(row, dt, Ci, Co, nsplit)
    wg.h.x, wg.h.mode = x.ptr(), capi.SRC_PLAIN
    if hmode != "plain":
        wg.h.mode, wg.h.relu = capi.SRC_BN, int(hmode == "bn_relu")
        wg.h.gamma, wg.h.beta = dev(P["gamma_h"], keep).data_ptr(), dev(P["beta_h"], keep).data_ptr()
        wg.h.inv_count, wg.h.eps = 1.0 / (B * Hi * Wi), R.EPS
        if hmode == "bn_eval":
            wg.h.rmean, wg.h.rvar = dev(P["rmean_h"], keep).data_ptr(), dev(P["rvar_h"], keep).data_ptr()
        else:
            wg.h.stats = shard0(R.channel_stats(P["x"]), keep).data_ptr()
    wg.g.x, wg.g.y, wg.g.mode = dy.ptr(), y.ptr(), capi.SRC_PLAIN
    if gmode == "bnbwd":
        wg.g.mode = capi.SRC_BNBWD
        wg.g.stats, wg.g.rstats = shard0(R.channel_stats(P["y"]), keep).data_ptr(), shard0(R.g_constants(P)[4], keep).data_ptr()
        wg.g.gamma = dev(P["gamma_g"], keep).data_ptr()
        wg.g.inv_count, wg.g.eps = 1.0 / (B * Ho * Wo), R.EPS
    dw = run_wgrad(wg, R.stated_instantiation(row, dt, Ci, Co, gmode == "bnbwd"), (x, dy, y))
    ratio = (dw - ref).abs() / E
    worst = float(ratio.max())
    RATIOS[dt] = max(RATIOS.get(dt, 0.0), worst)
    print(f"WGRAD_RATIO {dt} {R.case_id(case)} max|err|/E = {worst:.4f} (so far for {dt}: {RATIOS[dt]:.4f})")
    assert worst <= 1.0, f"{int((ratio > 1).sum())} elements beyond the bound, worst {worst:.3f} x E at {(ratio == ratio.max()).nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ stride-2 data gradient
@pytest.mark.parametrize("ops", ["none", "mask_y+red", "addend"])
@pytest.mark.parametrize("cap", ["", "16"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("chan", R.DGRAD_CHANNELS, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("shape", R.DGRAD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_stride2_data_gradient_equals_fp64_exactly(shape, chan, dt, cap, ops, monkeypatch):
    """stl_conv_forward with stuff = 1 (zero-stuffed gradient, flipped weights) on integer data against conv_transpose2d in fp64.
    The fp32 accumulator holds the exact integer; it is rounded to the output type once, so dx equals the reference rounded to
    that type (fp32: the integer itself; bf16: exact up to 256, which most sums are).  Planner-chosen tiles, once more with a grid
    cap of 16 blocks so that blocks walk several tiles.  With the epilogue operands the planner gives these layers: mask_y + red
    (dx = plain * [BN(x0) > 0], wherever the fp64 mask argument is further than 1e-3 from zero) and addend (dx = plain + addend)."""
    B, H, W = shape
    Ci, Co = chan
    T = "f32" if dt == "fp32" else "bf16"
    td = R.TORCH_DT[T]
    P = R.dgrad_problem(B, H, W, Ci, Co)
    Ho, Wo = P["g"].shape[1:3]
    if cap:
        monkeypatch.setenv("STL_CONV_GRID_CAP", cap)
    g = Guarded(P["g"].numel(), td, P["g"])
    wb = Guarded(Co * 9 * Ci, td, P["w"].reshape(Co, 9, Ci).flip(1).permute(2, 1, 0).contiguous())   # [Ci][tap][Co], as the chain test
    dx = Guarded(B * H * W * Ci, td)
    keep = []
    d = capi.Conv()
    d.dtype, d.B, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co = CODE[T], B, Ho, Wo, Co, H, W, Ci
    d.ks, d.stride, d.stuff, d.shape, d.TH, d.TW = 3, 1, 1, -1, 0, 0
    d.src.x, d.src.mode = g.ptr(), capi.SRC_PLAIN
    d.w, d.out = wb.ptr(), dx.ptr()
    want = P["dx"]
    arg = None
    if ops == "addend":
        ad = Guarded(B * H * W * Ci, td, P["addend"])
        keep.append(ad)
        d.addend = ad.ptr()
        want = want + P["addend"]
    if ops == "mask_y+red":
        x0 = Guarded(B * H * W * Ci, td, P["x0"])
        keep.append(x0)
        stored = x0.t.cpu().view(B, H, W, Ci)
        arg = R.dgrad_mask_argument(stored, P["gamma"], P["beta"])
        red = torch.zeros(capi.NSHARD * 2 * Ci, dtype=torch.float64, device="cuda")
        d.mask_y, d.red = x0.ptr(), red.data_ptr()
        d.mask_bn.x, d.mask_bn.mode, d.mask_bn.relu = x0.ptr(), capi.SRC_BN, 1
        d.mask_bn.stats = shard0(R.channel_stats(stored), keep).data_ptr()
        d.mask_bn.gamma, d.mask_bn.beta = dev(P["gamma"], keep).data_ptr(), dev(P["beta"], keep).data_ptr()
        d.mask_bn.inv_count, d.mask_bn.eps = 1.0 / (B * H * W), R.EPS
        want = want * (arg > 0)
    rc, err = launch("stl_conv_forward", d)
    assert rc == 0, err
    got = dx.t.cpu().view(B, H, W, Ci)
    assert not torch.isnan(got).any()
    assert dx.bands_intact() and g.bands_intact() and wb.bands_intact() and all(k.bands_intact() for k in keep if isinstance(k, Guarded))
    want = want.to(td)   # one rounding of the exact integer
    if arg is None:
        bad = (got != want).nonzero()
        assert torch.equal(got, want), f"{len(bad)} of {want.numel()} elements differ, first (b, y, x, ci) = {bad[0].tolist()}"
    else:
        sure = arg.abs() > 1e-3
        assert float((~sure).double().mean()) <= 0.01
        assert torch.equal(got[sure], want[sure]), f"{int((got[sure] != want[sure]).sum())} elements differ"
        assert bool(((got == want) | (got == 0) | (got == P["dx"].to(td)))[~sure].all())   # near the threshold: open or closed
        r = red.view(capi.NSHARD, 2, Ci).sum(0).cpu()
        assert torch.equal(r[0], got.double().reshape(-1, Ci).sum(0))   # r1 = sum of the stored dx: integers, exact

