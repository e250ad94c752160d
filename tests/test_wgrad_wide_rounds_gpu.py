"""GPU: the wide 1x1 weight-gradient kernel (wgrad64_kernel): its shared pixel walk for g and h, and its two schedules -- one
tile per barrier pair (the default) and rounds of two tiles (STL_WGRAD64_TILES=2).

1. Integer data, both schedules: the summed slabs EQUAL the fp64 reference for every length of a block's walk (1, 2, 3, 4, 5 and
   7 or more tiles: full rounds, a last round short by one tile, and blocks with a single tile), under NaN guard bands.
2. Real-valued transformed sources: every single slab of the rounds of two is bit-for-bit what one tile per round writes, so the
   summation order, and with it the training result, is the same in both.
3. The layer1 channel pairs with a BatchNorm-backward gradient against the fp64 bound of tests/wgrad_ref.py.
Every case is one launch per arm on a map of about a hundred pixels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from stlpose_amd import capi  # noqa: E402
from tests import wgrad_ref as R  # noqa: E402
from tests.test_wgrad_exact_gpu import (Guarded, dev, exact_device, grid_orders, launch, run_wgrad, shard0, wgrad_params,  # noqa: E402
                                        xform_device)

ENV = "STL_WGRAD64_TILES"
WIDE_ROWS = [row for row in R.TILES if row[0] in ("p1a", "p1b")]   # 4x9 (7 tiles), 13x9 (2), 5x4 (18), 1x128 (26), 128x1 (9), 6x7 (6), 5x3 (24), 16x8 (3)
PAIRS = [(64, 64), (128, 64), (96, 72), (64, 256), (256, 64)]      # (Ci, Co): one chunk, two, chunk tails, and the two layer1 pairs
WIDE_TYPES = ("bf16", "mixed")


def splits(npt):
    """nsplit values at which blocks walk 1, 2, 3, 4, 5 and (nsplit 1) all tiles of the problem."""
    return sorted({n for n in (1, 2, 3, 4, 5, npt) if n <= npt})


def walk_lengths(npt, nsplit):
    return {len(range(b, npt, nsplit)) for b in range(nsplit)}


def test_split_sweep_reaches_every_remainder_of_a_round():
    """The sweep below holds, over the eight tiles, walks of 1, 2, 3, 4, 5 and 7 or more tiles: for rounds of two (and of three)
    tiles that is every remainder of the last round, full rounds before it, and single-tile blocks."""
    assert sorted(row[3] for row in WIDE_ROWS) == [2, 3, 6, 7, 9, 18, 24, 26]
    lengths = set()
    for row in WIDE_ROWS:
        for ns in splits(row[3]):
            lengths |= walk_lengths(row[3], ns)
    assert {1, 2, 3, 4, 5, 6, 7} <= lengths and max(lengths) == 26
    for nt in (2, 3):
        assert {(n % nt, n >= nt) for n in lengths} >= {(r, full) for r in range(nt) for full in (False, True)} - {(0, False)}


def rounds_arg(name):
    """Tiles per round the launched instantiation reports: the argument behind TY (absent: 1)."""
    a = name.rstrip(">").split("<")[1].split(",")
    return int(a[6]) if len(a) > 6 else 1


EXACT = [(row, dt, Ci, Co) for row in WIDE_ROWS for dt in WIDE_TYPES for Ci, Co in PAIRS]


@pytest.mark.parametrize("tiles", [None, "2"], ids=["one-tile", "rounds-of-2"])
@pytest.mark.parametrize("case", EXACT, ids=R.case_id)
def test_wide_rounds_equal_fp64_exactly(case, tiles, monkeypatch):
    row, dt, Ci, Co = case
    T, TY = R.TYPES[dt]
    monkeypatch.delenv(ENV, raising=False)
    if tiles:
        monkeypatch.setenv(ENV, tiles)
    expect = R.stated_instantiation(row, dt, Ci, Co, 0)
    assert expect[0] == "wgrad64_kernel"
    h, g, gy, ref = exact_device(row[0], Ci, Co, T, TY)
    for nsplit in splits(row[3]):
        for xcd in grid_orders(expect, Ci, Co):
            monkeypatch.setenv("STL_WGRAD_XCD", xcd)
            wg = wgrad_params(row, dt, Ci, Co, nsplit)
            wg.h.x, wg.h.mode = h.ptr(), capi.SRC_PLAIN
            wg.g.x, wg.g.y, wg.g.mode = g.ptr(), gy.ptr(), capi.SRC_PLAIN
            dw = run_wgrad(wg, expect, (h, g, gy))   # asserts the kernel, no NaN in the slabs, all guard bands intact
            assert rounds_arg(capi.lib().stl_last_kernel().decode()) == int(tiles or 1)
            bad = (dw != ref).nonzero()
            assert torch.equal(dw, ref), f"nsplit {nsplit} XCD={xcd}: {len(bad)} of {ref.numel()} elements differ, first (co, tap, ci) = " \
                                         f"{bad[0].tolist()}: {float(dw[tuple(bad[0])])} != {float(ref[tuple(bad[0])])}"


# ------------------------------------------------------------------------------------------------ transformed sources
def xform_launch(row, dt, Ci, Co, nsplit, hmode, gmode, keep):
    """The launch parameters of one transformed-source problem (as section 3 of tests/test_wgrad_exact_gpu.py builds them) and
    the guarded tensors it reads."""
    geom = row[0]
    B, Hi, Wi, ks, s = R.GEOMS[geom]
    Ho, Wo = R.out_hw(geom)
    P = R.xform_problem(geom, Ci, Co, dt)
    x, dy, y = xform_device(geom, Ci, Co, dt)
    wg = wgrad_params(row, dt, Ci, Co, nsplit)
    wg.h.x, wg.h.mode = x.ptr(), capi.SRC_PLAIN
    if hmode != "plain":
        wg.h.mode, wg.h.relu = capi.SRC_BN, int(hmode == "bn_relu")
        wg.h.gamma, wg.h.beta = dev(P["gamma_h"], keep).data_ptr(), dev(P["beta_h"], keep).data_ptr()
        wg.h.inv_count, wg.h.eps = 1.0 / (B * Hi * Wi), R.EPS
        wg.h.stats = shard0(R.channel_stats(P["x"]), keep).data_ptr()
    wg.g.x, wg.g.y, wg.g.mode = dy.ptr(), y.ptr(), capi.SRC_PLAIN
    if gmode == "bnbwd":
        wg.g.mode = capi.SRC_BNBWD
        wg.g.stats, wg.g.rstats = shard0(R.channel_stats(P["y"]), keep).data_ptr(), shard0(R.g_constants(P)[4], keep).data_ptr()
        wg.g.gamma = dev(P["gamma_g"], keep).data_ptr()
        wg.g.inv_count, wg.g.eps = 1.0 / (B * Ho * Wo), R.EPS
    return wg, (x, dy, y)


def run_slabs(wg, expect, inputs):
    """One launch into NaN slabs between guard bands; returns the slabs [nsplit][Co][tap][Ci] as written (fp32 bits, CPU) and the
    tiles per round of the kernel that ran."""
    part = Guarded(wg.nsplit * wg.Co * wg.Ci, torch.float32)
    wg.partial = part.ptr()
    rc, err = launch("stl_conv_wgrad", wg)
    assert rc == 0, err
    name = capi.lib().stl_last_kernel().decode()
    assert R.parse_kernel_name(name) == expect, f"launched {name}, the case expects {expect}"
    assert not torch.isnan(part.t).any(), "slab elements not written, or NaN read from a guard band"
    assert part.bands_intact(), "write outside the slabs"
    for t in inputs:
        assert t.bands_intact()
    return part.t.view(torch.int32).view(wg.nsplit, wg.Co, wg.Ci).cpu(), rounds_arg(name)


def bitwise_cases():
    """Every tile with every nsplit of the sweep (each remainder class of a round many times over), the channel pairs and types
    rotating; g BNBWD beside h bn_relu, and per tile one PLAIN gradient beside h bn."""
    out = []
    for r, row in enumerate(WIDE_ROWS):
        for s, ns in enumerate(splits(row[3])):
            Ci, Co = PAIRS[(r + s) % len(PAIRS)]
            out.append((row, WIDE_TYPES[(r + s) % 2], Ci, Co, ns, "bn_relu", "bnbwd"))
        Ci, Co = PAIRS[(r + 2) % len(PAIRS)]
        out.append((row, WIDE_TYPES[(r + 1) % 2], Ci, Co, min(2, row[3]), "bn", "plain"))
    return out


@pytest.mark.parametrize("case", bitwise_cases(), ids=R.case_id)
def test_wide_rounds_keep_every_slab_bitwise(case, monkeypatch):
    """Slab by slab (not their sum), rounds of two tiles write the bits of one tile per round (the default; spelled
    STL_WGRAD64_TILES=1 and left unset)."""
    row, dt, Ci, Co, nsplit, hmode, gmode = case
    expect = R.stated_instantiation(row, dt, Ci, Co, gmode == "bnbwd")
    keep = []
    wg, inputs = xform_launch(row, dt, Ci, Co, nsplit, hmode, gmode, keep)
    monkeypatch.setenv(ENV, "1")
    one, nt_one = run_slabs(wg, expect, inputs)
    monkeypatch.delenv(ENV)
    dflt, nt_dflt = run_slabs(wg, expect, inputs)
    monkeypatch.setenv(ENV, "2")
    new, nt_new = run_slabs(wg, expect, inputs)
    assert (nt_one, nt_dflt, nt_new) == (1, 1, 2), f"the arms ran {nt_one}, {nt_dflt} and {nt_new} tiles per round"
    assert torch.equal(one, dflt)
    diff = (one != new).nonzero()
    assert torch.equal(one, new), f"{len(diff)} of {one.numel()} slab elements differ in their bits, first (slab, co, ci) = {diff[0].tolist()}"


@pytest.mark.parametrize("tiles", [None, "2"], ids=["one-tile", "rounds-of-2"])
@pytest.mark.parametrize("dt", WIDE_TYPES)
@pytest.mark.parametrize("chan", [(256, 64), (64, 256)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_layer1_pair_with_bnbwd_within_fp64_bound(chan, dt, tiles, monkeypatch):
    """A layer1 channel pair (section 3 of tests/test_wgrad_exact_gpu.py stops at 128 channels), g BNBWD, h bn_relu, blocks of
    two and three tiles: |got - ref| <= E elementwise (tests/wgrad_ref.py: bound)."""
    monkeypatch.delenv(ENV, raising=False)
    if tiles:
        monkeypatch.setenv(ENV, tiles)
    Ci, Co = chan
    row = WIDE_ROWS[0]   # p1a, 4 x 9 tiles: 7 of them
    ref, E = R.xform_reference(row[0], Ci, Co, dt, "bn_relu", "bnbwd")
    keep = []
    wg, inputs = xform_launch(row, dt, Ci, Co, 3, "bn_relu", "bnbwd", keep)
    dw = run_wgrad(wg, R.stated_instantiation(row, dt, Ci, Co, 1), inputs)
    ratio = (dw - ref).abs() / E
    worst = float(ratio.max())
    print(f"WGRAD_RATIO {dt} {Ci}x{Co} max|err|/E = {worst:.4f}")
    assert worst <= 1.0, f"{int((ratio > 1).sum())} elements beyond the bound, worst {worst:.3f} x E at {(ratio == ratio.max()).nonzero()[0].tolist()}"
