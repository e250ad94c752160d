"""CPU: the fp64 references, the error bound and the case tables of tests/wgrad_ref.py, which tests/test_wgrad_exact_gpu.py
holds the weight-gradient and stride-2 data-gradient kernels against."""
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_ref as R


@pytest.mark.parametrize("shape", [(2, 7, 5, 8, 12, 3, 2), (3, 6, 5, 12, 8, 3, 1), (2, 7, 5, 8, 16, 1, 2)])
def test_wgrad_fp64_matches_autograd_cpu(shape):
    B, H, W, Ci, Co, ks, s = shape
    pad = 1 if ks == 3 else 0
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Co, Ci, ks, ks, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=s, padding=pad)
    go = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(go)
    got = R.wgrad_fp64(x.permute(0, 2, 3, 1), go.permute(0, 2, 3, 1), ks, s)
    ref = w.grad.permute(0, 2, 3, 1).reshape(Co, ks * ks, Ci)   # [Co][tap][Ci]
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    # and one element from the definition: dw[co][tap][ci] = sum g[pixel][co] h[pixel * stride + tap - pad][ci]
    co, ky, kx, ci = Co - 1, ks - 1, 0, Ci - 1
    acc = 0.0
    for b in range(B):
        for oy in range(y.shape[2]):
            for ox in range(y.shape[3]):
                iy, ix = oy * s + ky - pad, ox * s + kx - pad
                if 0 <= iy < H and 0 <= ix < W:
                    acc += float(go[b, co, oy, ox] * x[b, ci, iy, ix])
    assert abs(float(got[co, ky * ks + kx, ci]) - acc) < 1e-10


@pytest.mark.parametrize("shape", [(2, 7, 5, 8, 16), (2, 6, 8, 16, 8)])
def test_dgrad_fp64_matches_autograd_cpu(shape):
    B, H, W, Ci, Co = shape
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Co, Ci, 3, 3, generator=gen, dtype=torch.float64)
    y = F.conv2d(x, w, stride=2, padding=1)
    go = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(go)
    got = R.dgrad_fp64(go.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1), H, W)
    assert torch.allclose(got, x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_integer_problems_are_exact_cpu():
    """The premise of the exact tests: operands from {-3..3} without 0, at most 4096 pixels, so that every weight-gradient
    sum is an integer below 2^24, and the same in every storage type."""
    for geom in R.GEOMS:
        h, g, dw = R.exact_problem(geom, 8, 8)
        for t in (h, g):
            assert set(t.unique().tolist()) <= set(float(v) for v in R.INT_VALUES)
            for td in R.TORCH_DT.values():
                assert torch.equal(t.to(td).double(), t)
        assert torch.equal(dw, dw.round()) and float(dw.abs().max()) < 2 ** 24 and float(dw.abs().max()) > 0
    for B, H, W in R.DGRAD_SHAPES:
        P = R.dgrad_problem(B, H, W, 32, 32)
        assert torch.equal(P["dx"], P["dx"].round()) and float((P["dx"].abs() + 3).max()) < 2 ** 24
        # bf16 holds integers up to 256: a sum of at most 4 * 128 products of deviation 14 / 3 has deviation ~106, so nearly all
        # data-gradient elements are exact in bf16 too and a lost product of +-1 changes the stored value
        big = R.dgrad_problem(B, H, W, 128, 128)["dx"]
        assert float((big.abs() <= 256).double().mean()) > 0.9


def test_tile_table_states_what_the_rules_give_cpu():
    """Every figure a TILES row states (tile count, NVH bucket per kernel, refusals) against the rules of wgrad.hip."""
    for row in R.TILES:
        geom, TH, TW, npt, nvh = row
        ks, s = R.GEOMS[geom][3:]
        assert TH * TW <= 128 and npt == R.tiles_per_problem(geom, TH, TW), row
        for dt, C in (("fp32", 32), ("bf16", 32), ("mixed", 32), ("bf16", 64), ("mixed", 64)):
            for gq in (0, 1):
                assert R.stated_instantiation(row, dt, C, C, gq) == R.instantiation(dt, ks, s, C, C, TH, TW, gq), (row, dt, C)
    for case in R.exact_cases() + R.xform_cases():
        row, dt, Ci, Co, ns = case[:5]
        assert 1 <= ns <= row[3]


def test_case_tables_cover_every_instantiation_cpu():
    """The exact cases (PLAIN gradient: GQ = 0) and the transformed-source cases (BNBWD: GQ = 1) together reach every
    instantiation of wgrad_kernel / wgrad64_kernel that stl_conv_wgrad can launch."""
    want = R.reachable_instantiations()
    assert len(want) == 56   # 24 (3x3, 8 waves) + 20 (1x1, 4 waves; bf16 NVH 18 unreachable) + 8 (64-channel 3x3) + 4 (wide 1x1)
    got = {R.stated_instantiation(c[0], c[1], c[2], c[3], 0) for c in R.exact_cases()}
    got |= {R.stated_instantiation(c[0], c[1], c[2], c[3], c[6] == "bnbwd") for c in R.xform_cases()}
    assert None not in got
    assert want - got == set(), sorted(want - got)
    assert got - want == set()
    assert {i for i in want if i[4] == 0} <= {R.stated_instantiation(c[0], c[1], c[2], c[3], 0) for c in R.exact_cases()}


def test_exact_cases_cover_the_issue_cpu():
    cases = R.exact_cases()
    for dt in R.TYPES:
        assert {(c[2], c[3]) for c in cases if c[1] == dt} == set(R.CHANNELS)
    for geom in R.GEOMS:    # every geometry: nsplit 1, 2 and tiles, in every type
        for dt in R.TYPES:
            mine = [c for c in cases if c[0][0] == geom and c[1] == dt]
            assert any(c[4] == 1 for c in mine) and any(c[4] == 2 for c in mine) and any(c[4] == c[0][3] > 2 for c in mine), (geom, dt)
    npts = {row[3] for row in R.TILES}
    assert {1, 2, 3} <= npts and any(n >= 5 and n % 2 for n in npts)
    assert any(r[1] == 1 for r in R.TILES) and any(r[2] == 1 for r in R.TILES)
    for geom in ("tiny1", "tiny2"):   # a tile that spans three images or more across the separator rows
        Ho = R.out_hw(geom)[0]
        assert any(r[0] == geom and r[1] >= 8 and r[1] >= 2 * (Ho + 1) + 1 for r in R.TILES)
    for r in R.TILES:
        Ho, Wo = R.out_hw(r[0])
        B = R.GEOMS[r[0]][0]
        if r[0] == "s1" and r[2] < Wo and Wo % r[2] and (B * (Ho + 1)) % r[1]:
            break
    else:
        raise AssertionError("no tile that divides neither Wo nor B (Ho + 1)")
    assert (R.TILES[4], "bf16", 64, 64) in R.refused_cases() and R.TILES[4][:3] == ("s1", 1, 128)


@pytest.mark.parametrize("dt", ["fp32", "bf16", "mixed"])
@pytest.mark.parametrize("hmode,gmode", [("bn_relu", "bnbwd"), ("bn", "plain"), ("bn_eval", "bnbwd"), ("plain", "bnbwd")])
def test_bound_holds_for_an_emulation_and_catches_swapped_constants_cpu(dt, hmode, gmode):
    """E is neither wrong nor vacuous: a float32 emulation of the kernel (constants and transform in fp32, operands rounded to
    T, fp32 accumulation) stays within E of the fp64 reference; a reference with two channels' constants swapped does not."""
    geom, Ci, Co = "s2odd", 16, 24
    B, Hi, Wi, ks, s = R.GEOMS[geom]
    T, TY = R.TYPES[dt]
    P = R.xform_problem(geom, Ci, Co, dt)
    ref, E = R.xform_reference(geom, Ci, Co, dt, hmode, gmode)
    assert float(E.min()) > 0
    f32 = lambda t: t.float()
    x, y, dy = f32(P["x"]), f32(P["y"]), f32(P["dy"])
    if hmode == "plain":
        h = x
    else:
        a, b = (f32(c) for c in R.h_constants(P, hmode))
        h = a * x + b
        if hmode == "bn_relu":
            h = h.clamp_min(0.0)
    if gmode == "plain":
        g = dy
    else:
        a, b, cm, cs = (f32(c) for c in R.g_constants(P)[:4])
        g = a * dy + (b * y + (cm + cs))
    h, g = h.to(R.TORCH_DT[T]).float(), g.to(R.TORCH_DT[T]).float()
    emu = torch.nn.grad.conv2d_weight(h.permute(0, 3, 1, 2), (Co, Ci, ks, ks), g.permute(0, 3, 1, 2), stride=s, padding=1)
    emu = emu.permute(0, 2, 3, 1).reshape(Co, ks * ks, Ci).double()
    ratio = float(((emu - ref).abs() / E).max())
    assert ratio <= 1.0, ratio
    if dt != "fp32":
        assert ratio > 1e-3   # not vacuous: the emulation uses a fair part of it
    # constants of channels 0 and 1 swapped, on the side that has a transform
    swap = lambda c: torch.cat([c[1:2], c[0:1], c[2:]])
    if gmode == "bnbwd":
        wrong = R.transformed(P, hmode, gmode, gconst=tuple(swap(c) for c in R.g_constants(P)[:4]))
        bad = (slice(0, 2), slice(None), slice(None))
    else:
        wrong = R.transformed(P, hmode, gmode, hconst=tuple(swap(c) for c in R.h_constants(P, hmode)))
        bad = (slice(None), slice(None), slice(0, 2))
    err = (R.wgrad_fp64(wrong[0], wrong[1], ks, s) - ref).abs()
    assert float((err[bad] / E[bad]).max()) > 10.0 and float((err[bad] > E[bad]).double().mean()) > 0.5
    if hmode == "bn_relu":   # a dropped ReLU is outside the bound as well
        a, b = R.h_constants(P, hmode)
        norelu = R.wgrad_fp64(a * P["x"].double() + b, R.transformed(P, hmode, gmode)[1], ks, s)
        assert float(((norelu - ref).abs() > E).double().mean()) > 0.5


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dgrad_mask_argument_is_rarely_near_zero_cpu(dt):
    """The masked data-gradient case leaves out elements whose fp64 mask argument is within 1e-3 of zero: at most 1 %."""
    td = R.TORCH_DT["f32" if dt == "fp32" else "bf16"]
    for B, H, W in R.DGRAD_SHAPES:
        for Ci, Co in R.DGRAD_CHANNELS:
            P = R.dgrad_problem(B, H, W, Ci, Co)
            arg = R.dgrad_mask_argument(P["x0"].to(td), P["gamma"], P["beta"])
            assert float((arg.abs() <= 1e-3).double().mean()) <= 0.01
            assert 0.2 < float((arg > 0).double().mean()) < 0.8   # a real mask: neither all open nor all closed
