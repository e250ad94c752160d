"""GPU: every kernel family behind stl_conv_forward (conv_core_kernel, conv_ws_kernel, conv1x1_kernel, conv_r2_kernel) against
the fp64 CPU references of tests/conv_ref.py -- forward convolutions, block-end (BNADD) sources with src_out, and stride-1 data
gradients (BNBWD source) with their epilogue operand sets.

Exact tests: every operand, per-channel constant and intermediate is a small integer (tests/conv_ref.py says why, and asserts the
conditions on the CPU), so out, src_out, out_stats and red must EQUAL the reference; there is no tolerance in this file.  Every
case states the kernel instantiation it expects and compares it with stl_last_kernel(); every tensor the launch touches lies
between NaN guard bands, and the outputs start as NaN, so that an element never written, a stray read and a stray write all show.
412 cases (400 launches compared, 12 refusals) run in 5 s on an MI355X, the fp64 references included (measured; the
references are computed once per problem and shared between the types, shapes and grids that run it)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from stlpose_amd import capi  # noqa: E402
from tests import conv_ref as R  # noqa: E402
from tests.gpu_guard import Guarded, launch  # noqa: E402

CODE = {"f32": capi.F32, "f32s": capi.F32, "bf16": capi.BF16, "f16": capi.F16}
F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def device_inputs(geom, Ci, Co, mode, ops, dt):
    """The integer problem on the device in the case's element types, each tensor between guard bands (never modified)."""
    P = R.problem(geom, Ci, Co, mode, ops)
    T, TY = R.TYPES[dt]
    td, tyd = R.TORCH_DT[T], R.TORCH_DT[TY]
    smode, relu, batch = R.MODES[mode]
    G = {"x": Guarded(P["x"].numel(), td, P["x"]), "w": Guarded(P["w"].numel(), td, P["w"])}
    if "y" in P:   # BNADD: the skip tensor (as the source); BNBWD: the raw conv output, a forward tensor
        G["y"] = Guarded(P["y"].numel(), tyd if smode == R.BNBWD else td, P["y"])
    for k in ("gamma", "beta", "bias", "mask_gamma", "mask_beta"):
        if k in P:
            G[k] = Guarded(P[k].numel(), F32, P[k])
    if "mean" in P:
        if batch:
            G["stats"] = Guarded(capi.NSHARD * 2 * Ci, F64, R.fabricated_sums(P["mean"]))
        else:
            G["rmean"], G["rvar"] = Guarded(Ci, F32, P["mean"]), Guarded(Ci, F32, torch.ones(Ci))
    if "c1" in P:
        G["rstats"] = Guarded(capi.NSHARD * 2 * Ci, F64, R.rstats_sums(P["c1"], P["c2"]))
    if "addend" in P:
        G["addend"] = Guarded(P["addend"].numel(), td, P["addend"])
    if "mask_y" in P:
        G["mask_y"] = Guarded(P["mask_y"].numel(), tyd, P["mask_y"])
        G["mask_stats"] = Guarded(capi.NSHARD * 2 * Co, F64, R.fabricated_sums(P["mask_mean"]))
    if "mask_z" in P:
        G["mask_z"] = Guarded(P["mask_z"].numel(), tyd, P["mask_z"])
    return G


def fill(row):
    """The stl_conv of a row (inputs only) and the tensors it points to."""
    geom, Ci, Co, dt, mode, ops, (kind, shape, TH, TW) = row[:7]
    B, Hi, Wi, ks, s = R.GEOMS[geom]
    Ho, Wo = R.out_hw(geom)
    T, TY = R.TYPES[dt]
    smode, relu, batch = R.MODES[mode]
    G = device_inputs(geom, Ci, Co, mode, ops, dt)
    given = R.row_desc(row)
    d = capi.Conv()
    d.dtype, d.B, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co, d.ks, d.stride = CODE[T], B, Hi, Wi, Ci, Ho, Wo, Co, ks, s
    d.shape, d.TH, d.TW, d.stuff = given.shape, given.TH, given.TW, given.stuff
    d.ydtype = CODE[TY] if TY != T else 0
    d.math = capi.MATH_BF16X3 if T == "f32s" else capi.MATH_NATIVE
    d.src.x, d.src.mode, d.src.relu, d.w = G["x"].ptr(), smode, relu, G["w"].ptr()
    if smode != R.PLAIN:
        d.src.gamma, d.src.inv_count, d.src.eps = G["gamma"].ptr(), R.INV_COUNT, 0.0
        if batch:
            d.src.stats = G["stats"].ptr()
        else:
            d.src.rmean, d.src.rvar = G["rmean"].ptr(), G["rvar"].ptr()
        if smode == R.BNBWD:
            d.src.y, d.src.rstats = G["y"].ptr(), G["rstats"].ptr()
        else:
            d.src.beta = G["beta"].ptr()
        if smode == R.BNADD:
            d.src.y = G["y"].ptr()
    opset = R.ops_of(ops)
    d.out_relu = int("relu" in opset)
    if "bias" in opset:
        d.bias = G["bias"].ptr()
    if "addend" in opset:
        d.addend = G["addend"].ptr()
    if "mask_z" in opset:
        d.mask_z = G["mask_z"].ptr()
    if "mask_y" in opset:
        P = R.problem(geom, Ci, Co, mode, ops)
        d.mask_y = d.mask_bn.x = G["mask_y"].ptr()
        d.mask_bn.mode, d.mask_bn.relu = capi.SRC_BN, int(P["mask_relu"])
        d.mask_bn.stats, d.mask_bn.gamma, d.mask_bn.beta = G["mask_stats"].ptr(), G["mask_gamma"].ptr(), G["mask_beta"].ptr()
        d.mask_bn.inv_count, d.mask_bn.eps = R.INV_COUNT, 0.0
    return d, G


def differing(got, want, what):
    bad = (got != want).nonzero()
    if len(bad) == 0:
        return ""
    i = tuple(bad[0].tolist())
    return f"{what}: {len(bad)} of {want.numel()} elements differ, first (b, y, x, c) = {list(i)}: {float(got[i])} != {float(want[i])}"


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_conv_equals_fp64_exactly(row, monkeypatch):
    geom, Ci, Co, dt, mode, ops, plan, cap, expect = row
    B, Hi, Wi, ks, s = R.GEOMS[geom]
    Ho, Wo = R.out_hw(geom)
    P = R.problem(geom, Ci, Co, mode, ops)
    td = R.TORCH_DT[R.TYPES[dt][0]]
    opset = R.ops_of(ops)
    if cap:
        monkeypatch.setenv("STL_CONV_GRID_CAP", cap)
    d, G = fill(row)
    out = Guarded(B * Ho * Wo * Co, td)
    outs = [out]
    d.out = out.ptr()
    if "src_out" in opset:
        zo = Guarded(B * Hi * Wi * Ci, td)
        d.src_out = zo.ptr()
        outs.append(zo)
    if "stats" in opset:
        st = Guarded(capi.NSHARD * 2 * Co, F64, torch.zeros(capi.NSHARD * 2 * Co))
        d.out_stats = st.ptr()
        outs.append(st)
    if "red" in opset:
        red = Guarded(capi.NSHARD * 2 * Co, F64, torch.zeros(capi.NSHARD * 2 * Co))
        d.red = red.ptr()
        outs.append(red)
    rc, err = launch("stl_conv_forward", d)
    assert rc == 0, err
    name = capi.lib().stl_last_kernel().decode()
    assert R.parse_kernel_name(name) == R.parse_kernel_name(expect), f"launched {name}, the case expects {expect}"
    got = out.t.cpu().view(B, Ho, Wo, Co)
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} output elements not written, or NaN read from a guard band"
    for t in list(G.values()) + outs:
        assert t.bands_intact(), "write outside a tensor"
    want = P["out"].to(td)   # one rounding of the exact integer (none at all within the limits tests/conv_ref.py asserts)
    assert torch.equal(got, want), differing(got, want, "out")
    if "src_out" in opset:
        z, zw = zo.t.cpu().view(B, Hi, Wi, Ci), P["v"].to(td)
        assert not torch.isnan(z).any(), f"{int(torch.isnan(z).sum())} src_out elements not written"
        assert torch.equal(z, zw), differing(z, zw, "src_out")
    if "stats" in opset:
        sums = st.t.cpu().view(capi.NSHARD, 2, Co).sum(0)
        assert torch.equal(sums, P["stats"]), f"out_stats: channels {(sums != P['stats']).nonzero()[:4].tolist()} differ"
    if "red" in opset:
        sums = red.t.cpu().view(capi.NSHARD, 2, Co).sum(0)
        assert torch.equal(sums, P["red"]), f"red: channels {(sums != P['red']).nonzero()[:4].tolist()} differ"


@pytest.mark.parametrize("row", R.REFUSED, ids=R.row_id)
def test_conv_refusals_launch_nothing(row):
    """A tile whose halo exceeds what the block shape can stage, a tile larger than the shape, forward-tensor types (ydtype) on a
    launch that is no data gradient, gradient sources in the forward-only types, and block-end sources where no kernel forms
    them: an error on the host that says which, and the NaN outputs stay NaN."""
    geom, Ci, Co, dt, mode, ops, plan, cap, message = row
    B, Hi, Wi = R.GEOMS[geom][:3]
    Ho, Wo = R.out_hw(geom)
    assert R.instantiation(R.row_desc(row)) is None
    d, G = fill(row)
    td = R.TORCH_DT[R.TYPES[dt][0]]
    out, zo = Guarded(B * Ho * Wo * Co, td), Guarded(B * Hi * Wi * Ci, td)
    d.out = out.ptr()
    if "src_out" in R.ops_of(ops):
        d.src_out = zo.ptr()
    rc, err = launch("stl_conv_forward", d)
    assert rc != 0 and message in err, err
    assert torch.isnan(out.t).all() and out.bands_intact() and torch.isnan(zo.t).all() and zo.bands_intact()
