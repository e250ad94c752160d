"""CPU: tests/conv_ref.py itself -- the fp64 references against float64 torch on non-integer data, what the exact comparison can
see, the exactness conditions of every table row, the restated planner and dispatch against stl_conv_plan and the source, and
the coverage of the instantiations the networks' launch plans run.  No GPU: plans are made on the host, nothing is launched."""
import collections
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stlpose_amd", "csrc")
EPS = 1e-5


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def batch_consts(y):
    f = y.reshape(-1, y.shape[-1])
    mean = f.mean(0)
    return mean, 1.0 / torch.sqrt(f.var(0, unbiased=False) + EPS)


# ------------------------------------------------------------------------------------------------ references against torch
@pytest.mark.parametrize("ks,stride,H,W", [(3, 1, 7, 5), (3, 2, 7, 6), (3, 2, 8, 5), (1, 1, 5, 4)])
def test_conv_fp64_is_the_headers_sum_cpu(ks, stride, H, W):
    """conv_fp64 (F.conv2d) against the sum of include/stlpose_hip.h written out tap by tap: the [Co][ky * ks + kx][Ci] layout."""
    x, w = rnd(2, H, W, 6, seed=1), rnd(5, ks * ks, 6, seed=2)
    pad = 1 if ks == 3 else 0
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    want = torch.zeros(2, Ho, Wo, 5, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            win = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            want += torch.einsum("bhwc,oc->bhwo", win, w[:, ky * ks + kx])
    torch.testing.assert_close(R.conv_fp64(x, w, ks, stride), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("ks", [3, 1])
def test_data_gradient_is_autograd_and_the_flipped_convolution_cpu(ks):
    """dgrad_fp64 (conv_transpose2d) = autograd of the forward convolution = conv_fp64 with dgrad_weights: what the kernel runs."""
    x, wf, g = rnd(2, 6, 5, 4, seed=3).requires_grad_(), rnd(7, ks * ks, 4, seed=4), rnd(2, 6, 5, 7, seed=5)
    (want,) = torch.autograd.grad(R.conv_fp64(x, wf, ks, 1), x, g)
    torch.testing.assert_close(R.dgrad_fp64(g, wf, ks), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.conv_fp64(g, R.dgrad_weights(wf), ks, 1), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("relu", [0, 1])
def test_bn_and_block_end_sources_are_batch_norm_cpu(relu):
    x, skip, gamma, beta = rnd(3, 5, 4, 6, seed=6) * 2 + 0.3, rnd(3, 5, 4, 6, seed=7), rnd(6, seed=8), rnd(6, seed=9)
    mean, rstd = batch_consts(x)
    bn = F.batch_norm(nchw(x), None, None, gamma, beta, True, 0.0, EPS).permute(0, 2, 3, 1)
    act = torch.relu if relu else (lambda t: t)
    torch.testing.assert_close(R.source_fp64(R.BN, relu, x, None, gamma, beta, mean, rstd=rstd), act(bn), rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(R.source_fp64(R.BNADD, relu, x, skip, gamma, beta, mean, rstd=rstd), act(bn + skip), rtol=1e-11, atol=1e-11)


def test_bnbwd_source_and_red_are_batch_norm_backward_cpu():
    """BNBWD on load against autograd through batch_norm, and the epilogue's red = (r1, r2) against the reductions of
    native_batch_norm_backward (grad_bias = sum dt, grad_weight = sum dt * yhat)."""
    y, dt, gamma = (rnd(3, 5, 4, 6, seed=10) * 1.5 + 0.2).requires_grad_(), rnd(3, 5, 4, 6, seed=11), rnd(6, seed=12)
    z = F.batch_norm(nchw(y), None, None, gamma, torch.zeros(6, dtype=torch.float64), True, 0.0, EPS)
    (want,) = torch.autograd.grad(z, y, nchw(dt))
    mean, rstd = batch_consts(y.detach())
    n = y.numel() // 6
    yhat = (y.detach() - mean) * rstd
    r1, r2 = dt.reshape(-1, 6).sum(0), (dt * yhat).reshape(-1, 6).sum(0)
    got = R.source_fp64(R.BNBWD, 0, dt, y.detach(), gamma, None, mean, r1 / n, r2 / n, rstd=rstd)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    out, _, red = R.epilogue_fp64(dt, mask_y=y.detach(), mask_gamma=gamma, mask_beta=torch.zeros(6, dtype=torch.float64), mask_mean=mean,
                                  mask_relu=False, want_red=True, mask_rstd=rstd)
    _, gw, gb = torch.ops.aten.native_batch_norm_backward(nchw(dt), nchw(y.detach()), gamma, None, None, mean, rstd, True, EPS, [True, True, True])
    torch.testing.assert_close(red[0], gb, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(red[1], gw, rtol=1e-11, atol=1e-11)
    assert torch.equal(out, dt)


def test_epilogue_gates_are_autograd_through_the_block_end_cpu():
    """Operand set 7 (addend, mask_y without ReLU, mask_z, red): the gradient reaching BN(y) + skip of z = relu(BN(y) + skip);
    operand set 1 (mask_y with ReLU): the gradient reaching BN(y) of relu(BN(y)).  Bias and output ReLU in the header's order."""
    y, skip = rnd(2, 4, 3, 5, seed=13) + 0.1, rnd(2, 4, 3, 5, seed=14)
    gamma, beta, acc, addend = rnd(5, seed=15), rnd(5, seed=16), rnd(2, 4, 3, 5, seed=17), rnd(2, 4, 3, 5, seed=18)
    mean, rstd = batch_consts(y)
    pre = (gamma * rstd * (y - mean) + beta + skip).requires_grad_()
    z = torch.relu(pre)
    (want,) = torch.autograd.grad(z, pre, acc + addend)
    out, _, red = R.epilogue_fp64(acc, addend=addend, mask_y=y, mask_gamma=gamma, mask_beta=beta, mask_mean=mean, mask_relu=False,
                                  mask_z=z.detach(), want_red=True, mask_rstd=rstd)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(red[1], (want * (y - mean) * rstd).reshape(-1, 5).sum(0), rtol=1e-11, atol=1e-11)
    bn = (gamma * rstd * (y - mean) + beta).requires_grad_()
    (want1,) = torch.autograd.grad(torch.relu(bn), bn, acc)
    out1, _, _ = R.epilogue_fp64(acc, mask_y=y, mask_gamma=gamma, mask_beta=beta, mask_mean=mean, mask_relu=True, mask_rstd=rstd)
    torch.testing.assert_close(out1, want1, rtol=1e-12, atol=1e-12)
    bias = rnd(5, seed=19)
    out2, stats, _ = R.epilogue_fp64(acc, bias=bias, out_relu=True, want_stats=True, round_to=torch.bfloat16)
    stored = torch.relu(acc + bias).to(torch.bfloat16).double()
    assert torch.equal(out2, stored)   # one rounding, after the ReLU; the statistics are those of the stored values
    assert torch.equal(stats, torch.stack([stored.reshape(-1, 5).sum(0), (stored * stored).reshape(-1, 5).sum(0)]))


# ------------------------------------------------------------------------------------------------ what the comparison sees
def test_single_faults_are_nonzero_integers_cpu():
    """Each fault alone changes the reference of a table problem by a non-zero INTEGER, so torch.equal cannot miss it: one
    dropped (pixel, tap, 8-channel vector), one separator row between two images read as the next image's row, one tile of a
    persistent loop skipped (seen as NaN in `out`, and in out_stats), a ReLU before instead of after the block-end add."""
    P = R.problem("m24", 256, 256, "plain", "stats")
    v, w, out = P["v"], P["w"], P["out"]
    b, oy, ox, tap, c0 = 1, 23, 17, 0, 248          # the last pixel of the last image, its upper-left tap, the last vector
    term = torch.einsum("c,oc->o", v[b, oy - 1, ox - 1, c0:c0 + 8], w[:, tap, c0:c0 + 8])
    assert bool((term == term.round()).all()) and int((term != 0).sum()) > 0
    # the row below image 0 is padding; a kernel that reads image 1's first row there adds, at the last pixel, its taps 6 and 7
    leak = torch.einsum("kc,okc->o", v[1, 0, 16:18], w[:, 6:8])
    assert bool((leak == leak.round()).all()) and int((leak != 0).sum()) > 0
    tile = out[0, 0:14]                                # one 14 x 18 tile of a 256-pixel block
    assert int((tile.reshape(-1, 256).sum(0) != 0).sum()) > 0 and int((tile != 0).sum()) > 0.9 * tile.numel()
    assert float((tile * tile).reshape(-1, 256).sum(0).min()) > 0   # every channel's sum of squares would miss it
    Z = R.problem("tiny1", 64, 64, "bnadd", "src_out+stats")
    early = (Z["gamma"] * (Z["x"] - Z["mean"]) + Z["beta"]).clamp_min(0.0) + Z["y"]
    diff = early - Z["v"]
    assert bool((diff == diff.round()).all()) and int((diff != 0).sum()) > 0.1 * diff.numel()
    dout = R.conv_fp64(early, Z["w"], 3, 1) - Z["acc"]
    assert bool((dout == dout.round()).all()) and int((dout != 0).sum()) > 0.5 * dout.numel()


def test_fabricated_statistics_are_exact_cpu():
    """The sums the cases fabricate give the integer mean and a variance of exactly 1 in the kernel's own fp64 arithmetic."""
    mean = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)
    s = R.fabricated_sums(mean).sum(0)
    m = s[0] * R.INV_COUNT
    assert torch.equal(m, mean) and torch.equal(s[1] * R.INV_COUNT - m * m, torch.ones(3, dtype=torch.float64))
    r = R.rstats_sums(mean, -mean).sum(0) * R.INV_COUNT
    assert torch.equal(r[0], mean) and torch.equal(r[1], -mean)
    assert bool((R.fabricated_sums(mean) == R.fabricated_sums(mean).round()).all())   # halves of multiples of 128


# ------------------------------------------------------------------------------------------------ the tables
def problems():
    return sorted({r[:3] + r[4:6] for r in R.ROWS})


def test_every_row_meets_the_exactness_conditions_cpu():
    for row in R.ROWS:
        R.check_exactness(*row[:6])
    # and the conditions bite: a bf16 row with every weight set would be rounded when stored
    geom, Ci, Co = "m24", 256, 256
    dense = R.conv_fp64(R.problem(geom, Ci, Co, "plain", "stats")["v"], torch.ones(Co, 9, Ci, dtype=torch.float64), 3, 1)
    assert float(dense.abs().max()) > R.OUT_LIMIT["bf16"]


def test_rows_state_what_the_restatement_gives_cpu():
    seen = set()
    for row in R.ROWS:
        geom, Ci, Co, dt, mode, ops, (kind, shape, TH, TW), cap, expect = row
        assert row[:8] not in seen, f"duplicate row {R.row_id(row)}"
        seen.add(row[:8])
        d = R.row_desc(row)
        assert R.kernel_name(R.instantiation(d)) == expect, R.row_id(row)
        assert R.parse_kernel_name(expect) == R.instantiation(d)
        assert (Ci % (4 if dt in ("f32", "f32s") else 8), Co % 8) == (0, 0)
        if R.use_1x1(d):
            assert (kind, shape, TH, TW) == ("planned", -1, 0, 0)
        elif kind == "planned":
            assert R.choose_plan(d) == (shape, TH, TW), R.row_id(row)
        else:   # a forced row launches only what the planner itself can emit for this descriptor
            assert kind == "forced" and R.emits(d, shape, TH, TW), R.row_id(row)
        if cap:   # the grid cap makes every block walk several tiles
            B = R.GEOMS[geom][0]
            Ho, Wo = R.out_hw(geom)
            npt = R.ceil_div(B * Ho * Wo, 256) if R.use_1x1(d) else R.ceil_div(B * (Ho + 1), TH) * R.ceil_div(Wo, TW)
            assert npt > int(cap), R.row_id(row)
    for row in R.REFUSED:   # refused by the launch, not for want of a plan
        d = R.row_desc(row)
        assert R.instantiation(d) is None, R.row_id(row)
        if row[6][0] == "planned" and not R.use_1x1(d):
            assert R.choose_plan(d) == row[6][1:], R.row_id(row)


def conv_of(d):
    from stlpose_amd import capi
    p = capi.Conv()
    p.dtype = {"f32": capi.F32, "f32s": capi.F32, "bf16": capi.BF16, "mixed": capi.BF16, "f16": capi.F16}[d.dt]
    p.math = capi.MATH_BF16X3 if d.dt == "f32s" else capi.MATH_NATIVE
    p.ydtype = capi.F16 if d.dt == "mixed" else 0
    p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co, p.ks, p.stride, p.stuff = d.B, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co, d.ks, d.stride, d.stuff
    p.src.mode, p.shape = d.mode, -1
    return p


def test_restated_planner_is_stl_conv_plan_cpu():
    """Every "planned" row, and every shape the restatement picks for the table's descriptors, against the library on the host."""
    from stlpose_amd import capi
    n = 0
    for row in R.ROWS + [r for r in R.REFUSED if r[6][0] == "planned" and r[3] != "f32s"]:   # (fp32x3 has no gradient plan)
        d = R.row_desc(row)
        if R.use_1x1(d):
            continue
        d.shape, d.TH, d.TW = -1, 0, 0
        p = conv_of(d)
        capi.call("stl_conv_plan", C.byref(p))
        assert (p.shape, p.TH, p.TW) == R.choose_plan(d), R.row_id(row)
        if row[6][0] == "planned":
            assert (p.shape, p.TH, p.TW) == row[6][1:], R.row_id(row)
            n += 1
    assert n > 150


def test_restatement_is_tied_to_the_source_cpu():
    """The figures the restatement copies: SHAPES, the LDS strides, the specialised operand sets, the kernels' parameter lists."""
    core = open(os.path.join(CSRC, "conv_core.hip")).read()
    body = re.search(r"constexpr Shape SHAPES\[NSHAPES\] = \{(.*?)\};", core, re.S).group(1)
    shapes = [tuple(int(v) for v in m.split(",")) for m in re.findall(r"\{([\d,\s]+)\}", body)]
    assert dict(enumerate(shapes)) == R.SHAPES
    assert int(re.search(r"constexpr int PSA = (\d+);", core).group(1)) == R.PSA
    r2 = open(os.path.join(CSRC, "conv_r2.inc")).read()
    assert int(re.search(r"constexpr int R2_PS = (\d+);", r2).group(1)) == R.R2_PS
    assert int(re.search(r"constexpr int R2_ROWF = (\d+);", r2).group(1)) == R.R2_ROWF
    common = open(os.path.join(CSRC, "conv_common.inc")).read()
    sets = re.search(r"return \(((?:eo == \d+(?: \|\| )?)+)\) \? eo : -1;", common).group(1)
    assert sorted(int(v) for v in re.findall(r"\d+", sets)) == [0, 1, 2, 7, 8, 48]
    for src, kernel in ((core, "conv_core_kernel"), (open(os.path.join(CSRC, "conv_ws.inc")).read(), "conv_ws_kernel"),
                        (open(os.path.join(CSRC, "conv1x1.inc")).read(), "conv1x1_kernel"), (r2, "conv_r2_kernel")):
        listed = re.search(r'stl_kname<T>\(nbuf, "%s", \{([^}]*)\}\)' % kernel, src).group(1)
        names = tuple("TY" if "stl_code<TY>" in a else a.strip() for a in listed.split(","))
        assert names == R.KERNEL_ARGS[kernel]


# ------------------------------------------------------------------------------------------------ coverage
def network_convs():
    """(plan name, stl_conv) of every stl_conv_forward launch of the networks' plans, built on the CPU."""
    from stlpose_amd import PoseHighResolutionNet, adain, vgg, vgg19_style
    from tests import launch_plans as LP
    out = []
    for dt, training in (("bf16", True), ("mixed", True), ("fp32", True), ("mixed", False), ("fp32x3", False)):
        m = PoseHighResolutionNet("w32", dt)
        m._pack(LP.CPU)
        e = m.engine(32, 384, 288, training)
        out += [(f"w32 {dt}", o[1]) for o in list(e.fwd_ops) + list(e.bwd_ops) if o[0] == "stl_conv_forward"]

    def listed(name, entries):
        return [(name, e[-1][0]._obj) for e in entries if e[-2] == "stl_conv_forward"]
    for dt in ("fp32", "bf16", "fp32x3"):
        m = vgg.VGGPerceptualLoss(resize=False, compute_dtype=dt)
        vgg.ready(m, LP.CPU)
        out += listed(f"vgg16 {dt}", m._plan(2, 32, 32, LP.CPU)[0].ops)
    m = vgg19_style.VGG19StyleLoss()
    vgg.ready(m, LP.CPU)
    sp = vgg19_style.StylePlan(m, 3, 32, 32, LP.CPU, 1, "batch", [0, 2], True)
    out += listed("vgg19", sp.trunk.ops) + listed("vgg19 backward", sp.bwd_ops)
    m = adain.AdaINStylizer()
    m._pack(LP.CPU)
    p = adain._Plan(m, 1, 32, 32, LP.CPU, True)
    return out + listed("adain", p.encode) + listed("adain", p.decode)


def test_every_instantiation_the_networks_run_is_in_the_tables_cpu():
    """HRNet-W32 at 384x288, batch 32 (training in bf16, mixed and fp32; evaluation in f16 -- the forward tensors of the mixed
    mode -- and fp32x3), VGG16, VGG19 with its backward pass, AdaIN: every stl_conv_forward descriptor mapped through the
    restatement.  The restated planner gives each its planned shape and tile; the set of instantiations is a subset of what the
    tables expect to launch; and what the dispatch can reach beyond the tables is exactly the NOT_PLANNED list."""
    covered = {r[8] for r in R.ROWS}
    run = collections.Counter()
    for plan, p in network_convs():
        d = R.desc_of_conv(p)
        if not R.use_1x1(d):
            free = R.desc(d.dt, d.B, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co, d.ks, d.stride, d.mode, d.ops, stuff=d.stuff)
            assert R.choose_plan(free) == (p.shape, p.TH, p.TW), (plan, vars(d))
        name = R.kernel_name(R.instantiation(d))
        assert name is not None, (plan, vars(d))
        run[name] += 1
    assert len(run) > 80
    assert set(run) <= covered, f"launched by a network, in no table row: {sorted(set(run) - covered)}"
    reachable = {R.kernel_name(i) for i in R.reachable_instantiations()}
    assert covered <= reachable
    assert not covered & set(R.NOT_PLANNED) and covered | set(R.NOT_PLANNED) == reachable, \
        (sorted(reachable - covered - set(R.NOT_PLANNED)), sorted(set(R.NOT_PLANNED) - reachable))


def test_tables_cover_the_issue_cpu():
    """The forms the tables must hold, by name: block shapes, staging buckets, filter residency, operand sets, types."""
    parsed = [(r, R.parse_kernel_name(r[8])) for r in R.ROWS]

    def has(base, T=None, rows=None, **want):
        names = R.KERNEL_ARGS[base]
        return any(b == base and (T is None or t == T) and all(a[names.index(k)] == v for k, v in want.items()) and (rows is None or rows(r))
                   for r, (b, t, a) in parsed)
    for T in ("f32", "f32s", "bf16", "f16"):
        for WM, WN, MT, NTW, NVA in ((4, 1, 2, 4, 3), (4, 1, 2, 4, 9), (8, 1, 4, 2, 6), (4, 2, 4, 2, 3), (4, 1, 2, 2, 3), (4, 1, 2, 2, 6), (8, 1, 2, 2, 3)):
            assert has("conv_core_kernel", T, KS=3, WM=WM, WN=WN, MT=MT, NTW=NTW, NVA=NVA, Q=0), (T, WM, WN, MT, NTW, NVA)
        for WM in (4, 8):   # shapes 4 and 8 with resident and with streamed filters
            assert has("conv_core_kernel", T, KS=3, WM=WM, WN=1, MT=2, NTW=2, WR=1) and has("conv_core_kernel", T, KS=3, WM=WM, WN=1, MT=2, NTW=2, NVA=3, WR=-1)
        assert has("conv_core_kernel", T, DB=1, EO=-1) and has("conv_core_kernel", T, EO=48) and has("conv_core_kernel", T, KS=1)
        assert has("conv_core_kernel", T, ZM=1, WM=4, WN=1, NTW=4) and has("conv_core_kernel", T, ZM=1, WN=2) and has("conv_core_kernel", T, ZM=1, WM=8)
        assert has("conv_core_kernel", T, ZM=1, WM=4, WN=1, NTW=2)
        for NTW, NVA in ((4, 3), (4, 9), (2, 3)):   # shapes 7 and 9
            assert has("conv_ws_kernel", T, NTW=NTW, NVA=NVA, EO=8) and has("conv_ws_kernel", T, NTW=NTW, NVA=NVA, EO=-1)
        assert has("conv1x1_kernel", T, Q=0, EO=8) and has("conv1x1_kernel", T, Q=0, EO=-1)
        assert has("conv1x1_kernel", T, ZM=1, EO=8) and has("conv1x1_kernel", T, ZM=1, EO=0)
    for T in ("bf16", "f16"):
        for MT, WM in ((4, 4), (2, 4), (2, 8)):
            for EO in (0, 8, 48):
                assert has("conv_r2_kernel", T, Q=0, EO=EO, MT=MT, WM=WM)
            assert has("conv_r2_kernel", T, ZM=1, EO=8, MT=MT, WM=WM) and has("conv_r2_kernel", T, ZM=1, EO=0, MT=MT, WM=WM)
    for T, TY in (("f32", 0), ("bf16", 1), ("bf16", 2)):   # stride-1 data gradients: fp32, bf16, mixed
        for EO in (0, 1, 2, 7, -1):
            # the EO forms of conv_core_kernel: the two-image 256 x 64 block (shape 3) and shape 8 with resident filters
            assert has("conv_core_kernel", T, KS=3, Q=1, ZM=0, TY=TY, EO=EO, DB=1), (T, TY, EO)
            assert has("conv_core_kernel", T, KS=3, Q=1, ZM=0, TY=TY, EO=EO, WM=8, WR=1), (T, TY, EO)
        for WM, WN, NTW in ((4, 1, 4), (4, 2, 2), (8, 1, 2), (4, 1, 2)):   # shapes 0, 2, 8 (streamed filters) and 4: run-time epilogue
            assert has("conv_core_kernel", T, KS=3, Q=1, ZM=0, TY=TY, EO=-1, WM=WM, WN=WN, NTW=NTW, DB=0), (T, TY, WM, WN, NTW)
        for EO in (0, 1, 2, 7):
            if T == "bf16" and EO >= 0:
                assert has("conv_r2_kernel", T, Q=1, ZM=0, TY=TY, EO=EO, MT=2, WM=4) and has("conv_r2_kernel", T, Q=1, ZM=0, TY=TY, EO=EO, MT=2, WM=8)
        assert has("conv_core_kernel", T, KS=1, Q=1, TY=TY) and has("conv1x1_kernel", T, Q=1, TY=TY, EO=2) and has("conv1x1_kernel", T, Q=1, TY=TY, EO=-1, ZM=0)
    # the fallbacks of conv_r2's shapes: a row that names shape 5 / 6 / 10 and lands on conv_core_kernel's 3 / 0 / 8
    for shape, (WM, WN, NTW) in ((5, (4, 2, 2)), (6, (4, 1, 4)), (10, (8, 1, 2))):
        assert has("conv_core_kernel", None, rows=lambda r: r[6][1] == shape, WM=WM, WN=WN, NTW=NTW), shape
    assert any(r[7] == "8" for r in R.ROWS) and {b for r, (b, t, a) in parsed if r[7] == "8"} == set(R.KERNEL_ARGS)
    assert {r[1] for r in R.ROWS} >= {4, 8, 20, 24, 40, 48, 64, 128, 256} and {r[2] for r in R.ROWS} >= {8, 40, 72, 96, 64, 128, 256}
    assert {"tiny1", "tiny2", "wide2", "s2odd", "s2even", "s1", "m24", "m24b4", "q24", "p1b"} <= {r[0] for r in R.ROWS}
    # a block-end source whose tile spans an image boundary: 2x2 maps, tiles taller than one image
    assert any(r[0] == "tiny1" and r[4].startswith("bnadd") and "src_out" in r[5] and r[6][2] > 3 for r in R.ROWS)
