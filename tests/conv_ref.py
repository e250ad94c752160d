"""Plain fp64 CPU references, a restatement of the host dispatch and the case tables for stl_conv_forward (conv_core.hip and
its includes conv_ws.inc, conv1x1.inc, conv_r2.inc).  Shared by tests/test_conv_exact_gpu.py (which runs the kernels) and
tests/test_conv_ref_cpu.py (which checks this file against float64 torch, the restatement against stl_conv_plan and the networks'
launch plans, and the exactness conditions of every row).  Needs no GPU.

Why the results are EXACT, transformed sources and epilogues included (common.cuh: src_consts, bn_mean_rstd, bn_affine, rsqrt_nr):

  mean, rstd   batch statistics: m = s0 * inv_count and var = fma(s1, inv_count, -m * m) in fp64, rstd = rsqrt_nr((float)(var + eps));
               eval mode: mean = rmean, rstd = rsqrt_nr(rvar + eps).  The cases choose eps = 0 and a variance of exactly 1: rvar = 1,
               or fabricated sums s0 = m / inv_count, s1 = (1 + m * m) / inv_count with inv_count = 2^-7 and an integer mean m (the
               kernel only multiplies by inv_count, so it need not be 1 / (B H W)); the sums are split over the STL_NSHARD shards in
               exact halves.  rsqrt_nr(1.0f) = r * fma(-0.5 r, r, 1.5) is 1.0f when the hardware estimate r is 1.0f, and also when it
               is one ulp above (1 - O(ulp^2) rounds to 1).
  BN           ca = gamma * rstd = gamma in {+-1, +-2}; cb = fma(-mean, ca, beta) = beta - m * gamma, an integer for an integer
               beta.  relu(ca * x + cb) of an integer x is a small integer.
  BNADD        relu(fma(ca, x, cb) + y) of integers x, y: a small integer; the same value is written to src_out.
  BNBWD        c1 = r1 * inv_count, c2 = r2 * inv_count with rstats r = c / inv_count for small integers c1, c2 (zero included);
               ca = gamma, cb = -gamma * c2, cc = gamma * fma(m, c2, -c1): v = fma(ca, dt, fma(cb, y, cc)) = gamma * (dt - c1 -
               c2 * (y - m)), a small integer -- exact in bf16 and f16.
  mask_bn      a = gamma, b = fma(-m, gamma, beta) with a HALF-integer beta: the mask argument a * y + b of an integer y is an
               integer plus one half, never zero; yhat = (y - m) * rstd = y - m.
  mask_z       an integer tensor without zeros: its sign is exact.  addend, bias: integers.

So every MFMA operand is a small integer (exact in bf16, f16, fp32, and in the split-bf16 form of fp32x3, whose low pieces are
zero), every fp32 accumulator holds an exact integer below 2^24 in any summation order, and the stored output is that integer
rounded once to the output type -- not at all, where |ref| <= 256 (bf16) or 2048 (f16).  out_stats and red are sums of integers
whose absolute sums stay below 2^24, exact in any fp32 partial order and in the fp64 atomics.  Each of these conditions is a
property of the reference alone; check_exactness() asserts them on the CPU for every row."""
import functools
import types

import torch
import torch.nn.functional as F

from tests import wgrad_ref as W

TORCH_DT = {"f32": torch.float32, "f32s": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# dt -> (T: element type of source, weights, output and MFMA operands; TY: type of the forward tensors a data gradient reads)
TYPES = {"f32": ("f32", "f32"), "f32s": ("f32s", "f32s"), "bf16": ("bf16", "bf16"), "f16": ("f16", "f16"), "mixed": ("bf16", "f16")}
OUT_LIMIT = {"f32": 2 ** 24, "f32s": 2 ** 24, "bf16": 256, "f16": 2048}   # integers up to here are stored without rounding
PLAIN, BN, BNBWD, BNADD = 0, 1, 2, 3
INV_COUNT = 2.0 ** -7

# name: (B, Hi, Wi, ks, stride).  The small maps of tests/wgrad_ref.py, and maps that fill the 256- and 512-pixel blocks.
GEOMS = dict(W.GEOMS)
GEOMS.update({
    "m24": (2, 24, 18, 3, 1),      # 50 virtual rows of 18: 256-pixel tiles are full, the last one ragged
    "m24b4": (4, 24, 18, 3, 1),    # 100 virtual rows: more than 8 tiles of 128 pixels, several 512-pixel tiles
    "q24": (3, 24, 18, 1, 1),      # 1x1: 1296 pixels = 5 blocks of 256 and 16 pixels
    "q24b8": (8, 24, 18, 1, 1),    # 1x1: 3456 pixels = 13.5 blocks of 256: more than 8 pixel blocks
    "m24b8": (8, 24, 18, 3, 1),    # 200 virtual rows: more than 8 tiles of 256 pixels (the grid cap of 8 blocks)
    "s2b4": (4, 24, 18, 3, 2),     # stride 2 -> 12x9 at B = 4
    "s2b16": (16, 24, 18, 3, 2),   # ... at B = 16: 208 virtual rows, more than 8 tiles of 128 pixels
    "big": (1, 256, 256, 3, 1),    # 65536 pixels: where the planner gives Co <= 32, Ci >= 128 the 512-pixel block
    "u13": (3, 7, 6, 3, 1),        # stuff = 1: the 7x6 gradient of a stride-2 convolution of 13x11 maps, zero-stuffed on load
    "u24": (2, 12, 9, 3, 1),       # ... 12x9 -> 24x18
})
STUFFED = {"u13": (13, 11), "u24": (24, 18)}   # geometries read with stuff = 1 -> (Ho, Wo), the size of the stride-2 conv's input


def out_hw(geom):
    B, Hi, Wi, ks, s = GEOMS[geom]
    if geom in STUFFED:
        return STUFFED[geom]
    pad = 1 if ks == 3 else 0
    return (Hi + 2 * pad - ks) // s + 1, (Wi + 2 * pad - ks) // s + 1


# ------------------------------------------------------------------------------------------------ references
def source_fp64(mode, relu, x, y=None, gamma=None, beta=None, mean=None, c1=None, c2=None, rstd=1.0):
    """The source transform of stl_src in float64.  x, y: [B, H, W, C]; the constants [C] (float64).
    PLAIN: x.  BN: [relu](gamma * rstd * (x - mean) + beta).  BNADD: [relu](BN(x) + y).
    BNBWD: gamma * rstd * (x - c1 - yhat * c2) with yhat = (y - mean) * rstd (x is the gradient dt, y the raw conv output)."""
    x = x.double()
    if mode == PLAIN:
        return x
    if mode == BNBWD:
        return gamma * rstd * (x - c1 - (y.double() - mean) * rstd * c2)
    v = gamma * rstd * (x - mean) + beta
    if mode == BNADD:
        v = v + y.double()
    return v.clamp_min(0.0) if relu else v


def conv_fp64(v, w, ks, stride):
    """out[b, oy, ox, co] = sum v[b, oy * stride + ky - pad, ox * stride + kx - pad, ci] * w[co][ky * ks + kx][ci], pad 1 (3x3)
    or 0 (1x1), in float64.  v: [B, H, W, Ci] NHWC, w: [Co][ks * ks][Ci].  Returns [B, Ho, Wo, Co]."""
    Co, taps, Ci = w.shape
    wt = w.double().reshape(Co, ks, ks, Ci).permute(0, 3, 1, 2).contiguous()
    o = F.conv2d(v.double().permute(0, 3, 1, 2).contiguous(), wt, stride=stride, padding=1 if ks == 3 else 0)
    return o.permute(0, 2, 3, 1).contiguous()


def dgrad_weights(wf):
    """The kernel-layout weights of the data gradient of a stride-1 convolution with forward weights wf [Cf_out][taps][Cf_in]:
    [Cf_in][taps, flipped][Cf_out], as test_stride2_data_gradient_equals_fp64_exactly lays them out."""
    return wf.flip(1).permute(2, 1, 0).contiguous()


def dgrad_fp64(g, wf, ks):
    """Data gradient of a stride-1 convolution in float64, by conv_transpose2d (independent of conv_fp64 and of the flip).
    g: [B, H, W, Cf_out], wf: [Cf_out][taps][Cf_in].  Returns [B, H, W, Cf_in]."""
    Cfo, taps, Cfi = wf.shape
    wt = wf.double().reshape(Cfo, ks, ks, Cfi).permute(0, 3, 1, 2).contiguous()   # (in, out, kh, kw) of conv_transpose2d
    o = F.conv_transpose2d(g.double().permute(0, 3, 1, 2).contiguous(), wt, stride=1, padding=1 if ks == 3 else 0)
    return o.permute(0, 2, 3, 1).contiguous()


def epilogue_fp64(acc, bias=None, addend=None, mask_y=None, mask_gamma=None, mask_beta=None, mask_mean=None, mask_relu=True,
                  mask_z=None, out_relu=False, want_stats=False, want_red=False, round_to=None, mask_rstd=1.0):
    """The epilogue in the kernel's order: + bias, + addend, the gate of mask_y's BatchNorm (where mask_relu: out = 0 where
    gamma * rstd * (mask_y - mean) + beta <= 0), the gate of mask_z (out = 0 where z <= 0), output ReLU, ONE rounding to the
    output type; then out_stats = per-channel (sum, sum of squares) of the STORED tensor, or red = (sum stored, sum stored * yhat)
    with yhat = (mask_y - mean) * rstd.  Returns (stored fp64, stats [2][Co] or None, red [2][Co] or None)."""
    f = acc.double().clone()
    if bias is not None:
        f = f + bias
    if addend is not None:
        f = f + addend.double()
    yhat = None
    if mask_y is not None:
        my = mask_y.double()
        if mask_relu:
            f = torch.where(mask_gamma * mask_rstd * (my - mask_mean) + mask_beta > 0, f, torch.zeros_like(f))
        yhat = (my - mask_mean) * mask_rstd
    if mask_z is not None:
        f = torch.where(mask_z.double() > 0, f, torch.zeros_like(f))
    if out_relu:
        f = f.clamp_min(0.0)
    if round_to is not None:
        f = f.to(round_to).double()
    flat = f.reshape(-1, f.shape[-1])
    stats = torch.stack([flat.sum(0), (flat * flat).sum(0)]) if want_stats else None
    red = torch.stack([flat.sum(0), (flat * yhat.reshape(flat.shape)).sum(0)]) if want_red else None
    return f, stats, red


# ------------------------------------------------------------------------------------------------ dispatch rules, restated
def ceil_div(a, b):
    return -(-a // b)


# id: (px, co, thr, ws, lthr, nva_max) -- SHAPES of conv_core.hip.  ws 1: conv_ws_kernel, 2: two LDS images, 3: conv_r2_kernel
SHAPES = {0: (128, 64, 256, 0, 256, 9), 1: (512, 32, 512, 0, 512, 6), 2: (256, 64, 512, 0, 512, 3), 3: (256, 64, 512, 2, 512, 3),
          4: (128, 32, 256, 0, 256, 6), 5: (256, 64, 512, 3, 512, 3), 6: (128, 64, 512, 3, 512, 2), 7: (128, 64, 512, 1, 256, 9),
          8: (256, 32, 512, 0, 512, 3), 9: (128, 32, 512, 1, 256, 3), 10: (256, 32, 512, 3, 512, 3)}
PSA, R2_PS, R2_ROWF = 96, 32, 576
EPI_BITS = {"mask_y": 1, "addend": 2, "mask_z": 4, "stats": 8, "bias": 16, "relu": 32}
OPERANDS = ("bias", "addend", "mask_y", "mask_z", "red")
_CODE = {"f32": 0, "f32s": 0, "bf16": 1, "f16": 2}


def desc(dt, B, Hi, Wi, Ci, Ho, Wo, Co, ks, stride, mode=PLAIN, ops=(), shape=-1, TH=0, TW=0, stuff=0):
    """What the dispatch looks at in an stl_conv: dt names dtype / ydtype / math, ops the non-null epilogue operands (of
    "bias", "addend", "mask_y", "mask_z", "red", "stats" = out_stats, "relu" = out_relu, "src_out")."""
    return types.SimpleNamespace(dt=dt, B=B, Hi=Hi, Wi=Wi, Ci=Ci, Ho=Ho, Wo=Wo, Co=Co, ks=ks, stride=stride, stuff=stuff, mode=mode,
                                 ops=frozenset(ops), shape=shape, TH=TH, TW=TW)


def epi_code(d):
    if ("red" in d.ops) != ("mask_y" in d.ops):
        return -1
    eo = sum(bit for name, bit in EPI_BITS.items() if name in d.ops)
    return eo if eo in (8, 1, 7, 2, 0, 48) else -1


def chunk(d):
    return 16 if d.dt in ("f32", "f32s") else 32


def lds_bytes(d, shape, TH, TW):
    """(LDS bytes, wres) of lds_bytes() in conv_core.hip."""
    ck, taps = chunk(d), d.ks * d.ks
    HR, HC = (TH - 1) * d.stride + d.ks, (TW - 1) * d.stride + d.ks
    nchunks = ceil_div(d.Ci, ck)
    cipad = nchunks * ck
    bco, ws = SHAPES[shape][1], SHAPES[shape][3]
    off = 3 * cipad * 4
    if ws == 3:
        off = (off + 4 * bco * 4 + 15) & ~15
        off += 2 * ((HR * HC * R2_PS + 15) & ~15)
        off = ((off + 1023) & ~1023) + bco * R2_ROWF
        return off + 512 * 4, 0
    off = (off + 4 * bco * 4 + 15) & ~15
    off_a = off
    off += ((HR * HC * PSA + 15) & ~15) * (2 if ws else 1)
    sz_b = bco * (taps * 64 + 32)
    resident = nchunks == 1 or (ws == 1 and off + sz_b * nchunks <= 150 * 1024)
    off += sz_b * nchunks if resident else sz_b * (2 if ws else 1)
    return max(off, off_a + 8 * 2 * bco * 4), int(resident)


def use_1x1(d):
    return d.ks == 1 and d.stride == 1 and not d.stuff and d.Ci >= 64 and d.Co >= 64


def r2_takes(d, cfg):
    if d.dt in ("f32", "f32s") or d.ks != 3 or d.stride != 1 or d.Ci % 32 != 0:
        return False
    if (d.Ci != 32) if cfg == 2 else (d.Ci < 64):
        return False
    eo = epi_code(d)
    if d.mode == BNADD:
        return eo in (8, 0)
    if d.mode == BNBWD:
        return cfg != 0 and d.dt != "f16" and eo in (0, 1, 2, 7)
    return eo in (8, 0, 48)


def choose_plan(d, r2_env=11):
    """(shape, TH, TW) of choose_plan() in conv_core.hip (default STL_CONV_R2 = 11, STL_CONV_DB on), or None: the admissibility
    rules of every block shape, the candidate tiles and the cost model, in the same order and the same double arithmetic."""
    best, best_cost = None, 1e300
    for shape in range(11):
        for th, tw, cost in candidates(d, shape, r2_env):
            if cost < best_cost:
                best, best_cost = (shape, th, tw), cost
    return best


def admits(d, shape, r2_env=11):
    """Whether choose_plan considers this block shape for the descriptor at all."""
    ck, f32 = chunk(d), d.dt in ("f32", "f32s")
    px, co, thr, ws, lthr, nva_max = SHAPES[shape]
    dgrad = d.mode == BNBWD
    pixels = d.B * d.Ho * d.Wo
    r2_side = bool(r2_env & (2 if dgrad else 1))
    deep_small = (d.stride == 1 and d.ks == 3 and d.Co >= 256 and pixels <= 16384 and
                  not ((r2_env & 8) and not f32 and d.Ci % 32 == 0 and d.Ci >= 64 and r2_side))
    want_ws = d.stride == 2 or deep_small
    wide_k = d.Co <= 32 and d.Ci >= 128 and d.stride == 1 and d.ks == 3 and not d.stuff and pixels >= 65536
    c32 = d.Co <= 32 and d.stride == 1 and d.ks == 3 and not wide_k
    if px > 128 and d.stride == 2:
        return False
    if (ws == 1) != want_ws:
        return False
    if want_ws and shape != (9 if deep_small else 7):
        return False
    if shape in (2, 3, 5, 6):
        db = d.ks == 3 and d.stride == 1 and d.Ci > ck
        r2 = db and r2_side and not f32 and d.Ci % 32 == 0 and d.Ci >= 64
        small_map = bool(r2_env & 8) and d.Co >= 256 and pixels <= 16384
        want = (6 if (dgrad or (r2_env & 4) or small_map) else 5) if r2 else (3 if db else 2)
        if shape != want:
            return False
    if shape in (1, 8, 10) and d.Co > 32:
        return False
    if shape in (4, 8, 10) and not c32:
        return False
    if c32 and shape not in (4, 8, 10):
        return False
    r2c32 = bool(r2_env & 16) and not f32 and d.Ci == 32 and r2_side
    if c32 and shape in (8, 10) and (shape == 10) != r2c32:
        return False
    if wide_k and shape != 1:
        return False
    return True


def candidates(d, shape, r2_env=11):
    """[(TH, TW, cost)] of the tiles choose_plan weighs for one block shape, in its order."""
    if not admits(d, shape, r2_env):
        return []
    px, co, thr, ws, lthr, nva_max = SHAPES[shape]
    wide_k = d.Co <= 32 and d.Ci >= 128 and d.stride == 1 and d.ks == 3 and not d.stuff and d.B * d.Ho * d.Wo >= 65536
    c32 = d.Co <= 32 and d.stride == 1 and d.ks == 3 and not wide_k
    vrows, nblk_co, out = d.B * (d.Ho + 1), ceil_div(d.Co, co), []
    for tw in range(min(d.Wo, 4), min(d.Wo, px) + 1):
        for frac in (4, 3, 2, 1):
            th = min((px // tw) * frac // 4, vrows)
            if th < 1:
                continue
            hr, hc = (th - 1) * d.stride + d.ks, (tw - 1) * d.stride + d.ks
            nva = ceil_div(hr * hc * 4, lthr)
            if nva > nva_max:
                continue
            lds = lds_bytes(d, shape, th, tw)[0]
            if (shape == 4 and lds > 40 * 1024 and nva <= 3) or (shape == 8 and lds > 80 * 1024):
                continue
            if (shape in (5, 6, 10) and lds > 76 * 1024) or lds > 158 * 1024:
                continue
            tiles = float(ceil_div(vrows, th) * ceil_div(d.Wo, tw))
            mfma = tiles * px * co * nblk_co * float(d.Ci) * d.ks * d.ks / 2048.0
            nbytes = tiles * nblk_co * (float(hr) * hc * d.Ci + float(co) * d.ks * d.ks * d.Ci) * 2.0 / 12.0
            cost = max(mfma, nbytes) + 0.3 * min(mfma, nbytes)
            waves = tiles * nblk_co * thr / 64.0
            if waves < 2048.0:
                cost *= 1.0 + 0.15 * min(2048.0 / waves - 1.0, 4.0)
            if c32 and shape == 4:
                cost *= 4.0
            if shape in (5, 6, 10):
                cost *= 0.98
            out.append((th, tw, cost))
    return out


R2_ENVS = (11, 0, 3, 31)   # STL_CONV_R2: the default, and the settings under which the suite's A/B tests plan and launch


def emits(d, shape, TH, TW):
    """Whether choose_plan could emit (shape, TH, TW) for the descriptor: an admitted shape and one of its candidate tiles, under
    the default planner or one of the STL_CONV_R2 settings of R2_ENVS."""
    return any((th, tw) == (TH, TW) for env in R2_ENVS for th, tw, _ in candidates(d, shape, env))


def _name(base, T, *args):
    return (base, T, tuple(int(a) for a in args))


def _core(T, TY, KS, WM, WN, MT, NTW, NVA, Q, PE, OCC=1, WR=-1, ZM=0, DB=0, EO=-1):
    return _name("conv_core_kernel", T, KS, WM, WN, MT, NTW, NVA, Q, PE, OCC, WR, ZM, _CODE[TY], DB, EO)


def _ws(T, TY, KS, MT, NTW, NVA, Q, EO):
    return _name("conv_ws_kernel", T, KS, MT, NTW, NVA, Q, _CODE[TY], EO)


def dispatch(T, TY, KS, Q, PE, EO, shape, nva, wres):
    """dispatch<T, TY, KS, Q, PE, EO>() of conv_core.hip."""
    EOC = EO if KS == 3 and (Q or EO == 48) else -1
    EOW = EO if KS == 3 and EO != 48 else -1
    OCC4 = 3 if Q or (T == "f32s" and KS == 3 and not PE) else 4
    if shape == 0 and nva <= 9:
        return _core(T, TY, KS, 4, 1, 2, 4, 3 if nva <= 3 else 9, Q, PE)
    if shape == 1 and nva <= 6:
        return _core(T, TY, KS, 8, 1, 4, 2, 6, Q, PE)
    if shape == 2 and nva <= 3:
        return _core(T, TY, KS, 4, 2, 4, 2, 3, Q, PE, 1)
    if shape == 3 and KS == 3 and nva <= 3 and not wres:
        return _core(T, TY, KS, 4, 2, 4, 2, 3, Q, PE, 1, 0, 0, 1, EOC)
    if shape == 8 and nva <= 3:
        return _core(T, TY, KS, 8, 1, 2, 2, 3, Q, PE, 4, 1, 0, 0, EOC) if wres else _core(T, TY, KS, 8, 1, 2, 2, 3, Q, PE, OCC4)
    if shape == 4 and nva <= 3:
        return _core(T, TY, KS, 4, 1, 2, 2, 3, Q, PE, 4, 1) if wres else _core(T, TY, KS, 4, 1, 2, 2, 3, Q, PE, OCC4)
    if shape == 4 and nva <= 6:
        return _core(T, TY, KS, 4, 1, 2, 2, 6, Q, PE, 3)
    if shape == 7 and nva <= 9:
        return _ws(T, TY, KS, 2, 4, 3 if nva <= 3 else 9, Q, -1 if Q else EOW)
    if shape == 9 and nva <= 3:
        return _ws(T, TY, KS, 2, 2, 3, Q, EOW)
    return None


def dispatch_bnadd(T, shape, nva):
    if nva > 3 or shape not in (0, 2, 3, 4, 8):
        return None
    WM, WN, MT, NTW, OCC = {0: (4, 1, 2, 4, 1), 2: (4, 2, 4, 2, 1), 3: (4, 2, 4, 2, 1), 4: (4, 1, 2, 2, 3), 8: (8, 1, 2, 2, 3)}[shape]
    return _core(T, T, 3, WM, WN, MT, NTW, 3, 1, 1, OCC, -1, 1)


def dispatch_r2(d, T, TY, shape):
    MT, WM = {5: (4, 4), 6: (2, 4), 10: (2, 8)}[shape]
    eo, FWD = epi_code(d), T == TY
    if d.mode == BNADD:
        return _name("conv_r2_kernel", T, _CODE[T], 1, 1, 8 if eo == 8 else 0, MT, WM) if FWD else None
    if d.mode == BNBWD:
        return _name("conv_r2_kernel", T, _CODE[TY], 1, 0, eo, MT, WM) if T != "f16" and MT == 2 and eo in (0, 1, 2, 7) else None
    return _name("conv_r2_kernel", T, _CODE[T], 0, 0, eo, MT, WM) if FWD and eo in (8, 0, 48) else None


def run_1x1(d, T, TY):
    eo = epi_code(d)
    if d.mode == BNADD:
        return _name("conv1x1_kernel", T, 2, 1, 4, _CODE[T], eo, 1) if T == TY and eo in (8, 0) else None
    if d.mode == BNBWD and T not in ("f16", "f32s"):
        return _name("conv1x1_kernel", T, 2, 1, 4, _CODE[TY], 2 if eo == 2 else -1, 0)
    return _name("conv1x1_kernel", T, 2, 0, 4, _CODE[T], 8 if eo == 8 else -1, 0) if T == TY else None


def instantiation(d):
    """(kernel, T, template arguments) that stl_conv_forward launches for the descriptor -- planned by choose_plan where it names
    no shape -- as stl_last_kernel() will name it, or None where the host refuses the launch.  Restates stl_conv_forward,
    conv_backend, dispatch, dispatch_bnadd (conv_core.hip), run_1x1 (conv1x1.inc) and r2_takes / dispatch_r2 (conv_r2.inc)."""
    T, TY = TYPES[d.dt]
    q = d.mode == BNBWD
    if d.mode == BNADD and (not ((d.ks == 3 and d.stride == 1 and not d.stuff) or use_1x1(d)) or set(d.ops) & set(OPERANDS)):
        return None
    if "src_out" in d.ops and d.mode != BNADD:
        return None
    if T == "f32s" and (q or d.stuff):
        return None
    if d.ks == 1 and (d.stride != 1 or d.stuff):
        return None
    refuse_type = (T != TY and not q) or (T in ("f16", "f32s") and q)
    if use_1x1(d):
        return None if refuse_type else run_1x1(d, T, TY)
    if 0 <= d.shape < 11 and d.TH > 0 and d.TW > 0:
        if d.TH * d.TW > SHAPES[d.shape][0]:
            return None
        shape, TH, TW = d.shape, d.TH, d.TW
    elif d.TH > 0 and d.TW > 0:
        if d.TH * d.TW > 128:
            return None
        shape, TH, TW = 0, d.TH, d.TW
    else:
        plan = choose_plan(d)
        if plan is None:
            return None
        shape, TH, TW = plan
    for r2_shape, cfg, fallback in ((5, 0, 3), (6, 1, 0), (10, 2, 8)):
        if shape == r2_shape and not r2_takes(d, cfg):
            shape = fallback
    px, co, thr, ws, lthr, nva_max = SHAPES[shape]
    nva = ceil_div(((TH - 1) * d.stride + d.ks) * ((TW - 1) * d.stride + d.ks) * 4, lthr)
    if nva > nva_max:
        return None
    lds, wres = lds_bytes(d, shape, TH, TW)
    if lds > 160 * 1024 or refuse_type:
        return None
    if ws == 3:
        return dispatch_r2(d, T, TY, shape)
    if d.mode == BNADD:
        return dispatch_bnadd(T, shape, nva)
    plain = not (set(d.ops) & set(OPERANDS))
    eo = epi_code(d)
    if d.ks == 3:
        if q:
            return dispatch(T, TY, 3, 1, 0, eo if eo in (1, 7, 2, 0) else -1, shape, nva, wres)
        if plain and eo == 8:
            return dispatch(T, T, 3, 0, 1, 8, shape, nva, wres)
        if not plain and eo == 48:
            return dispatch(T, T, 3, 0, 0, 48, shape, nva, wres)
        return dispatch(T, T, 3, 0, int(plain), -1, shape, nva, wres)
    if q:
        return dispatch(T, TY, 1, 1, 0, -1, shape, nva, wres)
    return dispatch(T, T, 1, 0, int(plain), -1, shape, nva, wres)


# template parameters of each kernel as stl_last_kernel() lists them after the element type
KERNEL_ARGS = {
    "conv_core_kernel": ("KS", "WM", "WN", "MT", "NTW", "NVA", "Q", "PE", "OCC", "WR", "ZM", "TY", "DB", "EO"),
    "conv_ws_kernel": ("KS", "MT", "NTW", "NVA", "Q", "TY", "EO"),
    "conv1x1_kernel": ("G", "Q", "OCC", "TY", "EO", "ZM"),
    "conv_r2_kernel": ("TY", "Q", "ZM", "EO", "MT", "WM"),
}


def parse_kernel_name(name):
    """stl_last_kernel() -> the tuple of instantiation()."""
    base, args = name.rstrip(">").split("<")
    a = args.split(",")
    assert base in KERNEL_ARGS and len(a) == 1 + len(KERNEL_ARGS[base]) and a[0] in _CODE, name
    return (base, a[0], tuple(int(v) for v in a[1:]))


def kernel_name(inst):
    return None if inst is None else f"{inst[0]}<{inst[1]},{','.join(str(v) for v in inst[2])}>"


def desc_of_conv(p):
    """desc() of a filled stl_conv (a ctypes stlpose_amd.capi.Conv)."""
    from stlpose_amd import capi
    if p.dtype == capi.F32:
        dt = "f32s" if p.math == capi.MATH_BF16X3 else "f32"
    elif p.dtype == capi.BF16:
        dt = "mixed" if p.ydtype == capi.F16 else "bf16"
    else:
        dt = "f16"
    ops = [n for n, f in (("bias", p.bias), ("addend", p.addend), ("mask_y", p.mask_y), ("mask_z", p.mask_z), ("red", p.red),
                          ("stats", p.out_stats), ("relu", p.out_relu), ("src_out", p.src_out)) if f]
    return desc(dt, p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co, p.ks, p.stride, p.src.mode, ops, p.shape, p.TH, p.TW, p.stuff)


# ------------------------------------------------------------------------------------------------ integer problems
MODES = {   # name: (stl_src mode, relu, batch statistics (else running statistics))
    "plain": (PLAIN, 0, 1), "bn": (BN, 0, 1), "bn_relu": (BN, 1, 1), "bn_eval": (BN, 0, 0), "bn_relu_eval": (BN, 1, 0),
    "bnadd": (BNADD, 1, 1), "bnadd_eval": (BNADD, 1, 0), "bnbwd": (BNBWD, 0, 1), "bnbwd_eval": (BNBWD, 0, 0),
}
WEIGHT_TERMS = 64   # non-zero weights per output element, on average: |out| stays near 5 sigma ~ 150 whatever K is
TERMS = {"big": 16}  # ... fewer on the large map, whose per-channel sums of squares run over 65536 pixels


def ops_of(ops):
    return frozenset(o for o in ops.split("+") if o)


def _pick(values, shape, gen):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]


def row_desc(row):
    """desc() of a table row as the test fills the stl_conv: a "planned" row leaves shape and tile to the library."""
    geom, Ci, Co, dt, mode, ops, (kind, shape, TH, TW) = row[:7]
    B, Hi, Wi, ks, s = GEOMS[geom]
    Ho, Wo = out_hw(geom)
    given = {"planned": (-1, 0, 0), "forced": (shape, TH, TW), "tile128": (-1, TH, TW)}[kind]
    return desc(dt, B, Hi, Wi, Ci, Ho, Wo, Co, ks, s, MODES[mode][0], ops_of(ops), *given, stuff=int(geom in STUFFED))


@functools.lru_cache(maxsize=None)
def problem(geom, Ci, Co, mode, ops):
    """Integer operands of one case and its fp64 reference, the same for every element type, block shape and grid (never
    modified).  Keys: x, y (BNADD: the skip; BNBWD: the raw conv output), w (kernel layout [Co][taps][Ci]; BNBWD: the flipped
    forward weights wf), gamma, beta, mean, c1, c2, bias, addend, mask_y, mask_gamma, mask_beta, mask_mean, mask_relu, mask_z;
    v (the transformed source = src_out), acc (the plain convolution), out, stats, red."""
    B, Hi, Wi, ks, s = GEOMS[geom]
    Ho, Wo = out_hw(geom)
    smode, relu, batch = MODES[mode]
    ops = ops_of(ops)
    gen = torch.Generator().manual_seed(9000 + 131 * Ci + 17 * Co + 7 * Hi + Wi + 1000 * smode + len(ops))
    P = {"mask_relu": "mask_z" not in ops}   # the fused block end gates by z alone (mask_bn.relu = 0)
    P["x"] = _pick(W.INT_VALUES, (B, Hi, Wi, Ci), gen)
    if smode != PLAIN:
        P["gamma"], P["beta"], P["mean"] = _pick((-2, -1, 1, 2), (Ci,), gen), _pick((-1, 0, 1), (Ci,), gen), _pick((-1, 0, 1), (Ci,), gen)
    if smode == BNADD:
        P["y"] = _pick((0, 0, 1, 2, 3), (B, Hi, Wi, Ci), gen)
    if smode == BNBWD:
        P["y"] = _pick((-2, -1, 0, 1, 2), (B, Hi, Wi, Ci), gen)
        P["c1"], P["c2"] = _pick((-1, 0, 1), (Ci,), gen), _pick((-1, 0, 1), (Ci,), gen)
    taps = ks * ks
    dens = min(1.0, TERMS.get(geom, WEIGHT_TERMS) / (taps * Ci))
    wshape = (Ci, taps, Co) if smode == BNBWD else (Co, taps, Ci)
    wsel = _pick((-1, 1), wshape, gen) * (torch.rand(wshape, generator=gen, dtype=torch.float64) < dens)
    P["v"] = source_fp64(smode, relu, P["x"], P.get("y"), P.get("gamma"), P.get("beta"), P.get("mean"), P.get("c1"), P.get("c2"))
    if smode == BNBWD:   # wsel = the forward weights [Cf_out = Ci][taps][Cf_in = Co]; reference by conv_transpose2d
        P["wf"], P["w"] = wsel, dgrad_weights(wsel)
        P["acc"] = W.dgrad_fp64(P["v"], wsel.reshape(Ci, 3, 3, Co), Ho, Wo) if geom in STUFFED else dgrad_fp64(P["v"], wsel, ks)
    else:
        P["w"] = wsel
        P["acc"] = conv_fp64(P["v"], wsel, ks, s)
    oshape = (B, Ho, Wo, Co)
    if "bias" in ops:
        P["bias"] = _pick((-3, -2, -1, 0, 1, 2, 3), (Co,), gen)
    if "addend" in ops:
        P["addend"] = _pick(W.INT_VALUES, oshape, gen)
    if "mask_y" in ops:
        P["mask_y"] = _pick((-2, -1, 0, 1, 2), oshape, gen)
        P["mask_gamma"], P["mask_mean"] = _pick((-2, -1, 1, 2), (Co,), gen), _pick((-1, 0, 1), (Co,), gen)
        P["mask_beta"] = _pick((-1.5, -0.5, 0.5, 1.5), (Co,), gen)
    if "mask_z" in ops:
        P["mask_z"] = _pick((-2, -1, 1, 1, 2, 3), oshape, gen)
    P["out"], P["stats"], P["red"] = epilogue_fp64(
        P["acc"], P.get("bias"), P.get("addend"), P.get("mask_y"), P.get("mask_gamma"), P.get("mask_beta"), P.get("mask_mean"),
        P["mask_relu"], P.get("mask_z"), "relu" in ops, "stats" in ops, "red" in ops)
    return P


def fabricated_sums(mean, batch=True):
    """[NSHARD = 2][2][C] fp64 sums that give exactly this integer mean and a variance of exactly 1 under inv_count = 2^-7, in
    exact halves over the two shards."""
    s = torch.stack([mean / INV_COUNT, (1.0 + mean * mean) / INV_COUNT])
    return torch.stack([s / 2, s / 2])


def rstats_sums(c1, c2):
    s = torch.stack([c1 / INV_COUNT, c2 / INV_COUNT])
    return torch.stack([s / 2, s / 2])


def check_exactness(geom, Ci, Co, dt, mode, ops):
    """The conditions under which the device result must EQUAL the reference, asserted on the reference alone."""
    P = problem(geom, Ci, Co, mode, ops)
    ks, s = GEOMS[geom][3:]
    smode = MODES[mode][0]
    for k in ("x", "y", "v", "w", "addend", "mask_y", "mask_z", "bias", "out"):   # integers; operands exact in every type
        if k in P:
            assert bool((P[k] == P[k].round()).all()), k
            assert k == "out" or float(P[k].abs().max()) <= 64, k
    if "mask_y" in P:   # the gate's argument is an integer plus one half; mask_z has no zero
        arg = P["mask_gamma"] * (P["mask_y"] - P["mask_mean"]) + P["mask_beta"]
        assert bool(((arg * 2).round() == arg * 2).all()) and float(arg.abs().min()) >= 0.5
    if "mask_z" in P:
        assert float(P["mask_z"].abs().min()) >= 1
    if geom in STUFFED:
        assert smode == BNBWD   # a zero-stuffed source is the gradient of a stride-2 convolution
        mag = W.dgrad_fp64(P["v"].abs(), P["wf"].abs().reshape(Ci, 3, 3, Co), *STUFFED[geom])
    else:
        mag = dgrad_fp64(P["v"].abs(), P["wf"].abs(), ks) if smode == BNBWD else conv_fp64(P["v"].abs(), P["w"].abs(), ks, s)
    for k in ("addend", "bias"):
        if k in P:
            mag = mag + P[k].abs()
    assert float(mag.max()) < 2 ** 24, "a partial sum of the accumulator could round"
    assert float(P["out"].abs().max()) <= OUT_LIMIT[TYPES[dt][0]], f"|ref| = {float(P['out'].abs().max())} is rounded when stored as {dt}"
    flat = P["out"].reshape(-1, Co)
    if P["stats"] is not None:
        assert float(flat.abs().sum(0).max()) < 2 ** 24 and float((flat * flat).sum(0).max()) < 2 ** 24
    if P["red"] is not None:
        yhat = (P["mask_y"] - P["mask_mean"]).reshape(-1, Co)
        assert float(flat.abs().sum(0).max()) < 2 ** 24 and float((flat * yhat).abs().sum(0).max()) < 2 ** 24


def row_id(row):
    geom, Ci, Co, dt, mode, ops, (kind, shape, TH, TW), cap = row[:8]
    return "-".join([geom, f"{Ci}x{Co}", dt, mode, ops or "none", f"{kind}{shape}.{TH}x{TW}"] + ([f"cap{cap}"] if cap else []))


def reachable_instantiations():
    """Every instantiation stl_conv_forward can launch for some descriptor, block shapes and tiles forced by the caller included:
    conv_backend's calls of dispatch / dispatch_bnadd / dispatch_r2 / run_1x1 over every type, kernel size, block shape, staging
    bucket and filter residency they accept."""
    out = set()
    for dt, (T, TY) in TYPES.items():
        fwd, bwd = T == TY, T in ("f32", "bf16")
        for shape in (0, 1, 2, 3, 4, 7, 8, 9):
            px, co, thr, ws, lthr, nva_max = SHAPES[shape]
            for nva in (3, 6, 9):
                if nva > nva_max:
                    continue
                for wres in (0, 1):
                    one = nva <= max(3, ceil_div(px * 4, lthr))   # a 1x1 halo is the tile itself
                    if fwd:
                        for PE in (0, 1):
                            out.add(dispatch(T, T, 3, 0, PE, -1, shape, nva, wres))
                            if one:
                                out.add(dispatch(T, T, 1, 0, PE, -1, shape, nva, wres))
                        out.add(dispatch(T, T, 3, 0, 1, 8, shape, nva, wres))
                        out.add(dispatch(T, T, 3, 0, 0, 48, shape, nva, wres))
                        out.add(dispatch_bnadd(T, shape, nva))
                    if bwd:
                        for EO in (-1, 0, 1, 2, 7):
                            out.add(dispatch(T, TY, 3, 1, 0, EO, shape, nva, wres))
                        if one:
                            out.add(dispatch(T, TY, 1, 1, 0, -1, shape, nva, wres))
        for mode in (PLAIN, BNADD, BNBWD):
            for ops in ("", "stats", "bias+relu", "mask_y+red", "addend", "mask_y+red+addend+mask_z", "bias"):
                for Ci in (32, 64):
                    d = desc(dt, 2, 24, 18, Ci, 24, 18, 64, 3, 1, mode, ops_of(ops))
                    for shape, cfg in ((5, 0), (6, 1), (10, 2)):
                        if r2_takes(d, cfg):
                            out.add(dispatch_r2(d, T, TY, shape))
                d = desc(dt, 2, 24, 18, 64, 24, 18, 64, 1, 1, mode, ops_of(ops))
                out.add(instantiation(d))
    out.discard(None)
    return out


# ------------------------------------------------------------------------------------------------ case tables
# (geometry, Ci, Co, dt, source mode, epilogue operands, (kind, shape, TH, TW), STL_CONV_GRID_CAP, the instantiation expected).
# kind "planned": the descriptor leaves shape and tile to the library, and (shape, TH, TW) is what stl_conv_plan gives it;
# "forced": the descriptor names them -- a combination choose_plan emits for this descriptor under one of R2_ENVS.  For the
# streaming 1x1 kernel, which has no plan, the triple is (-1, 0, 0).  One row at least per instantiation that a tiny problem
# reaches, then rows for the channel and geometry edges (ragged chunks of 32 / 16 input channels, 8 to 96 output channels against
# 32- and 64-channel blocks, tiles across image boundaries, the largest stride-2 halos), then rows that run under a grid cap of 8
# blocks, so that every block walks several tiles.  tests/test_conv_ref_cpu.py checks every column against the restatement above.
ROWS = [
    ("p1a", 96, 72, "bf16", "plain", "", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,0,4,1,-1,0>"),
    ("p1b", 96, 72, "bf16", "plain", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,0,4,1,8,0>"),
    ("q24", 96, 72, "bf16", "bnbwd", "", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,1,-1,0>"),
    ("q24b8", 96, 72, "bf16", "bnadd", "src_out", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,1,0,1>"),
    ("p1a", 96, 72, "bf16", "bnbwd_eval", "addend", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,1,2,0>"),
    ("p1b", 96, 72, "bf16", "bnadd", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,1,8,1>"),
    ("q24", 96, 72, "mixed", "bnbwd", "mask_y+red", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,2,-1,0>"),
    ("q24b8", 96, 72, "mixed", "bnbwd_eval", "addend", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,2,2,0>"),
    ("p1a", 96, 72, "f16", "plain", "bias", ("planned", -1, 0, 0), "", "conv1x1_kernel<f16,2,0,4,2,-1,0>"),
    ("p1b", 96, 72, "f16", "bn_relu", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f16,2,0,4,2,8,0>"),
    ("q24", 96, 72, "f16", "bnadd", "src_out", ("planned", -1, 0, 0), "", "conv1x1_kernel<f16,2,1,4,2,0,1>"),
    ("q24b8", 96, 72, "f16", "bnadd_eval", "src_out+stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f16,2,1,4,2,8,1>"),
    ("p1a", 96, 72, "f32", "plain", "relu+stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,0,4,0,-1,0>"),
    ("p1b", 96, 72, "f32", "bn_eval", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,0,4,0,8,0>"),
    ("q24", 96, 72, "f32", "bnbwd", "mask_y+red+addend", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,1,4,0,-1,0>"),
    ("q24b8", 96, 72, "f32", "bnadd_eval", "src_out", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,1,4,0,0,1>"),
    ("p1a", 96, 72, "f32", "bnbwd", "addend", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,1,4,0,2,0>"),
    ("p1b", 96, 72, "f32", "bnadd", "src_out+stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,1,4,0,8,1>"),
    ("q24", 96, 72, "f32s", "bn", "", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32s,2,0,4,0,-1,0>"),
    ("q24b8", 96, 72, "f32s", "bn_relu_eval", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32s,2,0,4,0,8,0>"),
    ("p1a", 96, 72, "f32s", "bnadd_eval", "src_out", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32s,2,1,4,0,0,1>"),
    ("p1b", 96, 72, "f32s", "bnadd", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32s,2,1,4,0,8,1>"),
    ("q24", 8, 8, "bf16", "bn_relu", "bias", ("forced", 0, 1, 17), "", "conv_core_kernel<bf16,1,4,1,2,4,3,0,0,1,-1,0,1,0,-1>"),
    ("q24b8", 8, 8, "bf16", "bn", "relu+stats", ("forced", 0, 1, 17), "", "conv_core_kernel<bf16,1,4,1,2,4,3,0,1,1,-1,0,1,0,-1>"),
    ("p1a", 8, 8, "bf16", "bnbwd", "", ("forced", 0, 3, 9), "", "conv_core_kernel<bf16,1,4,1,2,4,3,1,0,1,-1,0,1,0,-1>"),
    ("p1b", 8, 8, "mixed", "bnbwd", "", ("forced", 0, 4, 7), "", "conv_core_kernel<bf16,1,4,1,2,4,3,1,0,1,-1,0,2,0,-1>"),
    ("q24", 24, 40, "bf16", "plain", "bias+relu", ("planned", 2, 25, 10), "", "conv_core_kernel<bf16,1,4,2,4,2,3,0,0,1,-1,0,1,0,-1>"),
    ("q24b8", 24, 40, "bf16", "plain", "", ("planned", 2, 42, 6), "", "conv_core_kernel<bf16,1,4,2,4,2,3,0,1,1,-1,0,1,0,-1>"),
    ("p1a", 24, 40, "bf16", "bnbwd", "mask_y+red", ("planned", 2, 26, 9), "", "conv_core_kernel<bf16,1,4,2,4,2,3,1,0,1,-1,0,1,0,-1>"),
    ("p1b", 24, 40, "mixed", "bnbwd", "mask_y+red", ("planned", 2, 36, 7), "", "conv_core_kernel<bf16,1,4,2,4,2,3,1,0,1,-1,0,2,0,-1>"),
    ("q24", 8, 8, "bf16", "plain", "bias", ("planned", 1, 75, 6), "", "conv_core_kernel<bf16,1,8,1,4,2,6,0,0,1,-1,0,1,0,-1>"),
    ("q24b8", 8, 8, "bf16", "plain", "stats", ("planned", 1, 42, 9), "", "conv_core_kernel<bf16,1,8,1,4,2,6,0,1,1,-1,0,1,0,-1>"),
    ("p1a", 8, 8, "bf16", "bnbwd", "addend", ("planned", 1, 26, 9), "", "conv_core_kernel<bf16,1,8,1,4,2,6,1,0,1,-1,0,1,0,-1>"),
    ("p1b", 8, 8, "mixed", "bnbwd", "addend", ("planned", 1, 36, 7), "", "conv_core_kernel<bf16,1,8,1,4,2,6,1,0,1,-1,0,2,0,-1>"),
    ("m24", 128, 24, "bf16", "bn", "bias+relu", ("forced", 4, 1, 17), "", "conv_core_kernel<bf16,3,4,1,2,2,3,0,0,4,-1,0,1,0,-1>"),
    ("m24b4", 8, 8, "bf16", "bn", "bias+relu", ("forced", 4, 1, 17), "", "conv_core_kernel<bf16,3,4,1,2,2,3,0,0,4,1,0,1,0,-1>"),
    ("s1", 128, 24, "bf16", "bn", "", ("forced", 4, 3, 9), "", "conv_core_kernel<bf16,3,4,1,2,2,3,0,1,4,-1,0,1,0,-1>"),
    ("tiny1", 8, 8, "bf16", "bn", "", ("forced", 4, 15, 2), "", "conv_core_kernel<bf16,3,4,1,2,2,3,0,1,4,1,0,1,0,-1>"),
    ("m24", 128, 24, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 4, 1, 17), "", "conv_core_kernel<bf16,3,4,1,2,2,3,1,0,3,-1,0,1,0,-1>"),
    ("m24b4", 128, 24, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 4, 1, 17), "", "conv_core_kernel<bf16,3,4,1,2,2,3,1,0,3,-1,0,2,0,-1>"),
    ("s1", 8, 8, "bf16", "bnbwd", "mask_y+red+addend", ("forced", 4, 3, 9), "", "conv_core_kernel<bf16,3,4,1,2,2,3,1,0,4,1,0,1,0,-1>"),
    ("tiny1", 8, 8, "mixed", "bnbwd", "mask_y+red+addend", ("forced", 4, 15, 2), "", "conv_core_kernel<bf16,3,4,1,2,2,3,1,0,4,1,0,2,0,-1>"),
    ("m24", 8, 8, "bf16", "bnadd_eval", "src_out+stats", ("forced", 4, 1, 17), "", "conv_core_kernel<bf16,3,4,1,2,2,3,1,1,3,-1,1,1,0,-1>"),
    ("m24b4", 8, 8, "bf16", "bn", "bias", ("forced", 4, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,2,6,0,0,3,-1,0,1,0,-1>"),
    ("m24", 8, 8, "bf16", "bn", "stats", ("forced", 4, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,2,6,0,1,3,-1,0,1,0,-1>"),
    ("m24b4", 8, 8, "bf16", "bnbwd", "mask_y+red+addend", ("forced", 4, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,2,6,1,0,3,-1,0,1,0,-1>"),
    ("m24", 8, 8, "mixed", "bnbwd", "mask_z", ("forced", 4, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,2,6,1,0,3,-1,0,2,0,-1>"),
    ("m24b4", 256, 256, "bf16", "plain", "bias", ("planned", 6, 7, 18), "", "conv_core_kernel<bf16,3,4,1,2,4,3,0,0,1,-1,0,1,0,-1>"),
    ("s1", 128, 256, "bf16", "plain", "relu+stats", ("planned", 6, 14, 9), "", "conv_core_kernel<bf16,3,4,1,2,4,3,0,1,1,-1,0,1,0,-1>"),
    ("tiny1", 24, 40, "bf16", "bnbwd", "", ("planned", 0, 15, 2), "", "conv_core_kernel<bf16,3,4,1,2,4,3,1,0,1,-1,0,1,0,-1>"),
    ("m24", 64, 40, "mixed", "bnbwd", "mask_y+red+addend", ("planned", 6, 14, 9), "", "conv_core_kernel<bf16,3,4,1,2,4,3,1,0,1,-1,0,2,0,-1>"),
    ("tiny1", 24, 40, "bf16", "bnadd_eval", "src_out", ("planned", 0, 15, 2), "", "conv_core_kernel<bf16,3,4,1,2,4,3,1,1,1,-1,1,1,0,-1>"),
    ("m24", 24, 40, "bf16", "bn", "bias+relu", ("forced", 0, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,4,9,0,0,1,-1,0,1,0,-1>"),
    ("m24b4", 24, 40, "bf16", "plain", "relu+stats", ("forced", 0, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,4,9,0,1,1,-1,0,1,0,-1>"),
    ("m24", 24, 40, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 0, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,4,9,1,0,1,-1,0,1,0,-1>"),
    ("m24b4", 24, 40, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 0, 32, 4), "", "conv_core_kernel<bf16,3,4,1,2,4,9,1,0,1,-1,0,2,0,-1>"),
    ("m24b4", 24, 40, "bf16", "plain", "bias+relu", ("planned", 2, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,0,1,-1,0,1,0,-1>"),
    ("s1", 40, 72, "bf16", "bn_relu_eval", "bias", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,0,1,0,0,1,1,-1>"),
    ("m24", 40, 72, "bf16", "bn_relu_eval", "bias+relu", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,0,1,0,0,1,1,48>"),
    ("m24b4", 24, 40, "bf16", "plain", "stats", ("planned", 2, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,1,1,-1,0,1,0,-1>"),
    ("s1", 40, 72, "bf16", "plain", "relu+stats", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,1,1,0,0,1,1,-1>"),
    ("m24", 24, 40, "bf16", "bnbwd", "addend", ("planned", 2, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,-1,0,1,0,-1>"),
    ("m24b4", 24, 40, "mixed", "bnbwd", "addend", ("planned", 2, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,-1,0,2,0,-1>"),
    ("s1", 40, 72, "bf16", "bnbwd", "mask_z", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,-1>"),
    ("m24", 40, 72, "bf16", "bnbwd_eval", "", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,0>"),
    ("m24b4", 40, 72, "bf16", "bnbwd_eval", "mask_y+red", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,1>"),
    ("s1", 40, 72, "bf16", "bnbwd", "addend", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,2>"),
    ("m24", 40, 72, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,7>"),
    ("m24b4", 40, 72, "mixed", "bnbwd_eval", "mask_y+red+addend", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,2,1,-1>"),
    ("s1", 40, 72, "mixed", "bnbwd_eval", "", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,2,1,0>"),
    ("m24", 40, 72, "mixed", "bnbwd_eval", "mask_y+red", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,2,1,1>"),
    ("m24b4", 40, 72, "mixed", "bnbwd_eval", "addend", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,2,1,2>"),
    ("s1", 40, 72, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,2,1,7>"),
    ("m24", 24, 40, "bf16", "bnadd", "src_out", ("planned", 2, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,1,1,-1,1,1,0,-1>"),
    ("m24", 128, 24, "bf16", "plain", "bias+relu", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,0,4,-1,0,1,0,-1>"),
    ("m24b4", 8, 8, "bf16", "bn_eval", "bias", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,0,4,1,0,1,0,-1>"),
    ("s1", 8, 8, "bf16", "bn_relu_eval", "bias+relu", ("planned", 8, 26, 9), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,0,4,1,0,1,0,48>"),
    ("tiny1", 128, 24, "bf16", "plain", "stats", ("planned", 8, 15, 2), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,1,4,-1,0,1,0,-1>"),
    ("m24", 8, 8, "bf16", "plain", "stats", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,1,4,1,0,1,0,-1>"),
    ("m24b4", 128, 24, "bf16", "bnbwd", "mask_y+red", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,3,-1,0,1,0,-1>"),
    ("s1", 128, 24, "mixed", "bnbwd", "addend", ("planned", 8, 26, 9), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,3,-1,0,2,0,-1>"),
    ("tiny1", 8, 8, "bf16", "bnbwd", "mask_y+red+addend", ("planned", 8, 15, 2), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,-1>"),
    ("m24", 8, 8, "bf16", "bnbwd", "", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,0>"),
    ("m24b4", 8, 8, "bf16", "bnbwd", "mask_y+red", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,1>"),
    ("s1", 8, 8, "bf16", "bnbwd_eval", "addend", ("planned", 8, 26, 9), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,2>"),
    ("tiny1", 8, 8, "bf16", "bnbwd_eval", "mask_y+red+addend+mask_z", ("planned", 8, 15, 2), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,7>"),
    ("m24", 8, 8, "mixed", "bnbwd", "mask_z", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,-1>"),
    ("m24b4", 8, 8, "mixed", "bnbwd_eval", "", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,0>"),
    ("s1", 8, 8, "mixed", "bnbwd", "mask_y+red", ("planned", 8, 26, 9), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,1>"),
    ("tiny1", 8, 8, "mixed", "bnbwd", "addend", ("planned", 8, 15, 2), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,2>"),
    ("m24", 8, 8, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,7>"),
    ("m24b4", 8, 8, "bf16", "bnadd_eval", "src_out+stats", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,1,3,-1,1,1,0,-1>"),
    ("big", 128, 8, "bf16", "bn", "bias+relu", ("planned", 1, 13, 37), "", "conv_core_kernel<bf16,3,8,1,4,2,6,0,0,1,-1,0,1,0,-1>"),
    ("big", 128, 8, "bf16", "bn", "", ("planned", 1, 13, 37), "", "conv_core_kernel<bf16,3,8,1,4,2,6,0,1,1,-1,0,1,0,-1>"),
    ("q24", 8, 8, "f16", "bn_relu", "bias", ("forced", 0, 1, 17), "", "conv_core_kernel<f16,1,4,1,2,4,3,0,0,1,-1,0,2,0,-1>"),
    ("q24b8", 8, 8, "f16", "bn", "relu+stats", ("forced", 0, 1, 17), "", "conv_core_kernel<f16,1,4,1,2,4,3,0,1,1,-1,0,2,0,-1>"),
    ("p1a", 24, 40, "f16", "plain", "bias+relu", ("planned", 2, 26, 9), "", "conv_core_kernel<f16,1,4,2,4,2,3,0,0,1,-1,0,2,0,-1>"),
    ("p1b", 24, 40, "f16", "plain", "", ("planned", 2, 36, 7), "", "conv_core_kernel<f16,1,4,2,4,2,3,0,1,1,-1,0,2,0,-1>"),
    ("q24", 8, 8, "f16", "plain", "bias+relu", ("planned", 1, 75, 6), "", "conv_core_kernel<f16,1,8,1,4,2,6,0,0,1,-1,0,2,0,-1>"),
    ("q24b8", 8, 8, "f16", "plain", "", ("planned", 1, 42, 9), "", "conv_core_kernel<f16,1,8,1,4,2,6,0,1,1,-1,0,2,0,-1>"),
    ("s1", 128, 24, "f16", "plain", "bias", ("forced", 4, 3, 9), "", "conv_core_kernel<f16,3,4,1,2,2,3,0,0,4,-1,0,2,0,-1>"),
    ("tiny1", 8, 8, "f16", "plain", "bias", ("forced", 4, 15, 2), "", "conv_core_kernel<f16,3,4,1,2,2,3,0,0,4,1,0,2,0,-1>"),
    ("m24", 128, 24, "f16", "plain", "stats", ("forced", 4, 1, 17), "", "conv_core_kernel<f16,3,4,1,2,2,3,0,1,4,-1,0,2,0,-1>"),
    ("m24b4", 8, 8, "f16", "plain", "stats", ("forced", 4, 1, 17), "", "conv_core_kernel<f16,3,4,1,2,2,3,0,1,4,1,0,2,0,-1>"),
    ("s1", 8, 8, "f16", "bnadd", "stats", ("forced", 4, 3, 9), "", "conv_core_kernel<f16,3,4,1,2,2,3,1,1,3,-1,1,2,0,-1>"),
    ("m24b4", 8, 8, "f16", "bn_relu", "bias+relu", ("forced", 4, 32, 4), "", "conv_core_kernel<f16,3,4,1,2,2,6,0,0,3,-1,0,2,0,-1>"),
    ("m24", 8, 8, "f16", "bn", "relu+stats", ("forced", 4, 32, 4), "", "conv_core_kernel<f16,3,4,1,2,2,6,0,1,3,-1,0,2,0,-1>"),
    ("m24b4", 128, 256, "f16", "bn_relu", "bias", ("planned", 6, 7, 18), "", "conv_core_kernel<f16,3,4,1,2,4,3,0,0,1,-1,0,2,0,-1>"),
    ("s1", 128, 256, "f16", "bn_eval", "relu+stats", ("planned", 6, 14, 9), "", "conv_core_kernel<f16,3,4,1,2,4,3,0,1,1,-1,0,2,0,-1>"),
    ("tiny1", 24, 40, "f16", "bnadd", "src_out+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<f16,3,4,1,2,4,3,1,1,1,-1,1,2,0,-1>"),
    ("m24", 24, 40, "f16", "plain", "bias", ("forced", 0, 32, 4), "", "conv_core_kernel<f16,3,4,1,2,4,9,0,0,1,-1,0,2,0,-1>"),
    ("m24b4", 24, 40, "f16", "plain", "stats", ("forced", 0, 32, 4), "", "conv_core_kernel<f16,3,4,1,2,4,9,0,1,1,-1,0,2,0,-1>"),
    ("m24", 24, 40, "f16", "plain", "bias", ("planned", 2, 14, 18), "", "conv_core_kernel<f16,3,4,2,4,2,3,0,0,1,-1,0,2,0,-1>"),
    ("m24b4", 40, 72, "f16", "bn_relu", "bias", ("planned", 3, 14, 18), "", "conv_core_kernel<f16,3,4,2,4,2,3,0,0,1,0,0,2,1,-1>"),
    ("s1", 40, 72, "f16", "bn_eval", "bias+relu", ("planned", 3, 26, 9), "", "conv_core_kernel<f16,3,4,2,4,2,3,0,0,1,0,0,2,1,48>"),
    ("m24", 24, 40, "f16", "plain", "relu+stats", ("planned", 2, 14, 18), "", "conv_core_kernel<f16,3,4,2,4,2,3,0,1,1,-1,0,2,0,-1>"),
    ("m24b4", 40, 72, "f16", "plain", "relu+stats", ("planned", 3, 14, 18), "", "conv_core_kernel<f16,3,4,2,4,2,3,0,1,1,0,0,2,1,-1>"),
    ("s1", 24, 40, "f16", "bnadd_eval", "src_out", ("planned", 2, 26, 9), "", "conv_core_kernel<f16,3,4,2,4,2,3,1,1,1,-1,1,2,0,-1>"),
    ("m24", 128, 24, "f16", "bn_relu", "bias", ("planned", 8, 14, 18), "", "conv_core_kernel<f16,3,8,1,2,2,3,0,0,4,-1,0,2,0,-1>"),
    ("m24b4", 8, 8, "f16", "bn_relu_eval", "bias", ("planned", 8, 14, 18), "", "conv_core_kernel<f16,3,8,1,2,2,3,0,0,4,1,0,2,0,-1>"),
    ("s1", 8, 8, "f16", "plain", "bias+relu", ("planned", 8, 26, 9), "", "conv_core_kernel<f16,3,8,1,2,2,3,0,0,4,1,0,2,0,48>"),
    ("tiny1", 128, 24, "f16", "plain", "", ("planned", 8, 15, 2), "", "conv_core_kernel<f16,3,8,1,2,2,3,0,1,4,-1,0,2,0,-1>"),
    ("m24", 8, 8, "f16", "plain", "", ("planned", 8, 14, 18), "", "conv_core_kernel<f16,3,8,1,2,2,3,0,1,4,1,0,2,0,-1>"),
    ("m24b4", 8, 8, "f16", "bnadd", "src_out", ("planned", 8, 14, 18), "", "conv_core_kernel<f16,3,8,1,2,2,3,1,1,3,-1,1,2,0,-1>"),
    ("big", 128, 8, "f16", "bn_relu", "bias+relu", ("planned", 1, 13, 37), "", "conv_core_kernel<f16,3,8,1,4,2,6,0,0,1,-1,0,2,0,-1>"),
    ("big", 128, 8, "f16", "bn", "relu+stats", ("planned", 1, 13, 37), "", "conv_core_kernel<f16,3,8,1,4,2,6,0,1,1,-1,0,2,0,-1>"),
    ("q24", 4, 8, "f32", "plain", "bias", ("forced", 0, 1, 17), "", "conv_core_kernel<f32,1,4,1,2,4,3,0,0,1,-1,0,0,0,-1>"),
    ("q24b8", 4, 8, "f32", "plain", "stats", ("forced", 0, 1, 17), "", "conv_core_kernel<f32,1,4,1,2,4,3,0,1,1,-1,0,0,0,-1>"),
    ("p1a", 4, 8, "f32", "bnbwd", "addend", ("forced", 0, 3, 9), "", "conv_core_kernel<f32,1,4,1,2,4,3,1,0,1,-1,0,0,0,-1>"),
    ("p1b", 8, 72, "f32", "bn", "bias+relu", ("planned", 2, 36, 7), "", "conv_core_kernel<f32,1,4,2,4,2,3,0,0,1,-1,0,0,0,-1>"),
    ("q24", 8, 72, "f32", "plain", "relu+stats", ("planned", 2, 25, 10), "", "conv_core_kernel<f32,1,4,2,4,2,3,0,1,1,-1,0,0,0,-1>"),
    ("q24b8", 8, 72, "f32", "bnbwd", "addend", ("planned", 2, 42, 6), "", "conv_core_kernel<f32,1,4,2,4,2,3,1,0,1,-1,0,0,0,-1>"),
    ("p1a", 4, 8, "f32", "bn", "bias", ("planned", 1, 26, 9), "", "conv_core_kernel<f32,1,8,1,4,2,6,0,0,1,-1,0,0,0,-1>"),
    ("p1b", 4, 8, "f32", "bn", "", ("planned", 1, 36, 7), "", "conv_core_kernel<f32,1,8,1,4,2,6,0,1,1,-1,0,0,0,-1>"),
    ("q24", 4, 8, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 1, 75, 6), "", "conv_core_kernel<f32,1,8,1,4,2,6,1,0,1,-1,0,0,0,-1>"),
    ("m24b4", 32, 8, "f32", "bn", "bias", ("forced", 4, 1, 17), "", "conv_core_kernel<f32,3,4,1,2,2,3,0,0,4,-1,0,0,0,-1>"),
    ("s1", 4, 8, "f32", "bn_relu", "bias+relu", ("forced", 4, 3, 9), "", "conv_core_kernel<f32,3,4,1,2,2,3,0,0,4,1,0,0,0,-1>"),
    ("tiny1", 32, 8, "f32", "bn", "stats", ("forced", 4, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,2,3,0,1,4,-1,0,0,0,-1>"),
    ("m24", 4, 8, "f32", "bn", "stats", ("forced", 4, 1, 17), "", "conv_core_kernel<f32,3,4,1,2,2,3,0,1,4,1,0,0,0,-1>"),
    ("m24b4", 32, 8, "f32", "bnbwd", "mask_y+red+addend", ("forced", 4, 1, 17), "", "conv_core_kernel<f32,3,4,1,2,2,3,1,0,3,-1,0,0,0,-1>"),
    ("s1", 4, 8, "f32", "bnbwd", "mask_z", ("forced", 4, 3, 9), "", "conv_core_kernel<f32,3,4,1,2,2,3,1,0,4,1,0,0,0,-1>"),
    ("tiny1", 4, 8, "f32", "bnadd_eval", "stats", ("forced", 4, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,2,3,1,1,3,-1,1,0,0,-1>"),
    ("m24", 4, 8, "f32", "bn_relu", "bias", ("forced", 4, 32, 4), "", "conv_core_kernel<f32,3,4,1,2,2,6,0,0,3,-1,0,0,0,-1>"),
    ("m24b4", 4, 8, "f32", "bn", "relu+stats", ("forced", 4, 32, 4), "", "conv_core_kernel<f32,3,4,1,2,2,6,0,1,3,-1,0,0,0,-1>"),
    ("m24", 4, 8, "f32", "bnbwd", "", ("forced", 4, 32, 4), "", "conv_core_kernel<f32,3,4,1,2,2,6,1,0,3,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32", "plain", "bias", ("planned", 0, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,4,3,0,0,1,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32", "plain", "relu+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,4,3,0,1,1,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 0, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,4,3,1,0,1,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32", "bnadd_eval", "src_out+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,4,3,1,1,1,-1,1,0,0,-1>"),
    ("m24b4", 8, 72, "f32", "bn", "bias+relu", ("forced", 0, 32, 4), "", "conv_core_kernel<f32,3,4,1,2,4,9,0,0,1,-1,0,0,0,-1>"),
    ("m24", 8, 72, "f32", "bn", "", ("forced", 0, 32, 4), "", "conv_core_kernel<f32,3,4,1,2,4,9,0,1,1,-1,0,0,0,-1>"),
    ("m24b4", 8, 72, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 0, 32, 4), "", "conv_core_kernel<f32,3,4,1,2,4,9,1,0,1,-1,0,0,0,-1>"),
    ("m24b4", 8, 72, "f32", "bn", "bias+relu", ("planned", 2, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,0,0,1,-1,0,0,0,-1>"),
    ("s1", 20, 40, "f32", "bn_eval", "bias", ("planned", 3, 26, 9), "", "conv_core_kernel<f32,3,4,2,4,2,3,0,0,1,0,0,0,1,-1>"),
    ("m24", 20, 40, "f32", "bn_eval", "bias+relu", ("planned", 3, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,0,0,1,0,0,0,1,48>"),
    ("m24b4", 8, 72, "f32", "bn", "", ("planned", 2, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,0,1,1,-1,0,0,0,-1>"),
    ("s1", 20, 40, "f32", "bn", "stats", ("planned", 3, 26, 9), "", "conv_core_kernel<f32,3,4,2,4,2,3,0,1,1,0,0,0,1,-1>"),
    ("m24", 8, 72, "f32", "bnbwd", "mask_y+red+addend", ("planned", 2, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,-1,0,0,0,-1>"),
    ("m24b4", 20, 72, "f32", "bnbwd", "mask_y+red+addend", ("planned", 3, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,-1>"),
    ("s1", 20, 40, "f32", "bnbwd_eval", "", ("planned", 3, 26, 9), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,0>"),
    ("m24", 20, 40, "f32", "bnbwd_eval", "mask_y+red", ("planned", 3, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,1>"),
    ("m24b4", 20, 40, "f32", "bnbwd_eval", "addend", ("planned", 3, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,2>"),
    ("s1", 20, 72, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 3, 26, 9), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,7>"),
    ("m24", 8, 72, "f32", "bnadd", "src_out", ("planned", 2, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,1,1,-1,1,0,0,-1>"),
    ("s1", 32, 8, "f32", "bn_relu", "bias", ("planned", 8, 26, 9), "", "conv_core_kernel<f32,3,8,1,2,2,3,0,0,4,-1,0,0,0,-1>"),
    ("tiny1", 4, 8, "f32", "bn", "bias", ("planned", 8, 15, 2), "", "conv_core_kernel<f32,3,8,1,2,2,3,0,0,4,1,0,0,0,-1>"),
    ("m24", 4, 8, "f32", "bn", "bias+relu", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,0,0,4,1,0,0,0,48>"),
    ("m24b4", 32, 8, "f32", "bn", "relu+stats", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,0,1,4,-1,0,0,0,-1>"),
    ("s1", 4, 8, "f32", "plain", "", ("planned", 8, 26, 9), "", "conv_core_kernel<f32,3,8,1,2,2,3,0,1,4,1,0,0,0,-1>"),
    ("tiny1", 32, 8, "f32", "bnbwd", "", ("planned", 8, 15, 2), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,3,-1,0,0,0,-1>"),
    ("m24", 4, 8, "f32", "bnbwd_eval", "mask_y+red+addend", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,4,1,0,0,0,-1>"),
    ("m24b4", 4, 8, "f32", "bnbwd", "", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,4,1,0,0,0,0>"),
    ("s1", 4, 8, "f32", "bnbwd_eval", "mask_y+red", ("planned", 8, 26, 9), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,4,1,0,0,0,1>"),
    ("tiny1", 4, 8, "f32", "bnbwd_eval", "addend", ("planned", 8, 15, 2), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,4,1,0,0,0,2>"),
    ("m24", 4, 8, "f32", "bnbwd_eval", "mask_y+red+addend+mask_z", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,4,1,0,0,0,7>"),
    ("m24b4", 4, 8, "f32", "bnadd", "src_out+stats", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,1,3,-1,1,0,0,-1>"),
    ("big", 128, 8, "f32", "bn", "bias+relu", ("planned", 1, 13, 37), "", "conv_core_kernel<f32,3,8,1,4,2,6,0,0,1,-1,0,0,0,-1>"),
    ("big", 128, 8, "f32", "bn", "", ("planned", 1, 13, 37), "", "conv_core_kernel<f32,3,8,1,4,2,6,0,1,1,-1,0,0,0,-1>"),
    ("q24", 4, 8, "f32s", "bn", "bias+relu", ("forced", 0, 1, 17), "", "conv_core_kernel<f32s,1,4,1,2,4,3,0,0,1,-1,0,0,0,-1>"),
    ("q24b8", 4, 8, "f32s", "plain", "relu+stats", ("forced", 0, 1, 17), "", "conv_core_kernel<f32s,1,4,1,2,4,3,0,1,1,-1,0,0,0,-1>"),
    ("p1a", 8, 72, "f32s", "bn", "bias", ("planned", 2, 26, 9), "", "conv_core_kernel<f32s,1,4,2,4,2,3,0,0,1,-1,0,0,0,-1>"),
    ("p1b", 8, 72, "f32s", "bn", "", ("planned", 2, 36, 7), "", "conv_core_kernel<f32s,1,4,2,4,2,3,0,1,1,-1,0,0,0,-1>"),
    ("q24", 4, 8, "f32s", "bn", "bias", ("planned", 1, 75, 6), "", "conv_core_kernel<f32s,1,8,1,4,2,6,0,0,1,-1,0,0,0,-1>"),
    ("q24b8", 4, 8, "f32s", "bn", "", ("planned", 1, 42, 9), "", "conv_core_kernel<f32s,1,8,1,4,2,6,0,1,1,-1,0,0,0,-1>"),
    ("s1", 32, 8, "f32s", "bn_relu", "bias+relu", ("forced", 4, 3, 9), "", "conv_core_kernel<f32s,3,4,1,2,2,3,0,0,3,-1,0,0,0,-1>"),
    ("tiny1", 4, 8, "f32s", "bn_relu", "bias+relu", ("forced", 4, 15, 2), "", "conv_core_kernel<f32s,3,4,1,2,2,3,0,0,4,1,0,0,0,-1>"),
    ("m24", 32, 8, "f32s", "bn", "stats", ("forced", 4, 1, 17), "", "conv_core_kernel<f32s,3,4,1,2,2,3,0,1,4,-1,0,0,0,-1>"),
    ("m24b4", 4, 8, "f32s", "bn", "stats", ("forced", 4, 1, 17), "", "conv_core_kernel<f32s,3,4,1,2,2,3,0,1,4,1,0,0,0,-1>"),
    ("s1", 4, 8, "f32s", "bnadd_eval", "stats", ("forced", 4, 3, 9), "", "conv_core_kernel<f32s,3,4,1,2,2,3,1,1,3,-1,1,0,0,-1>"),
    ("m24b4", 4, 8, "f32s", "bn_relu", "bias+relu", ("forced", 4, 32, 4), "", "conv_core_kernel<f32s,3,4,1,2,2,6,0,0,3,-1,0,0,0,-1>"),
    ("m24", 4, 8, "f32s", "bn", "relu+stats", ("forced", 4, 32, 4), "", "conv_core_kernel<f32s,3,4,1,2,2,6,0,1,3,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32s", "bn_relu", "bias", ("planned", 0, 15, 2), "", "conv_core_kernel<f32s,3,4,1,2,4,3,0,0,1,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32s", "plain", "", ("planned", 0, 15, 2), "", "conv_core_kernel<f32s,3,4,1,2,4,3,0,1,1,-1,0,0,0,-1>"),
    ("tiny1", 8, 72, "f32s", "bnadd", "src_out+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<f32s,3,4,1,2,4,3,1,1,1,-1,1,0,0,-1>"),
    ("m24", 8, 72, "f32s", "plain", "bias", ("forced", 0, 32, 4), "", "conv_core_kernel<f32s,3,4,1,2,4,9,0,0,1,-1,0,0,0,-1>"),
    ("m24b4", 8, 72, "f32s", "plain", "stats", ("forced", 0, 32, 4), "", "conv_core_kernel<f32s,3,4,1,2,4,9,0,1,1,-1,0,0,0,-1>"),
    ("m24", 8, 72, "f32s", "bn_relu", "bias", ("planned", 2, 14, 18), "", "conv_core_kernel<f32s,3,4,2,4,2,3,0,0,1,-1,0,0,0,-1>"),
    ("m24b4", 20, 72, "f32s", "plain", "bias", ("planned", 3, 14, 18), "", "conv_core_kernel<f32s,3,4,2,4,2,3,0,0,1,0,0,0,1,-1>"),
    ("s1", 20, 40, "f32s", "plain", "bias+relu", ("planned", 3, 26, 9), "", "conv_core_kernel<f32s,3,4,2,4,2,3,0,0,1,0,0,0,1,48>"),
    ("m24", 8, 72, "f32s", "plain", "", ("planned", 2, 14, 18), "", "conv_core_kernel<f32s,3,4,2,4,2,3,0,1,1,-1,0,0,0,-1>"),
    ("m24b4", 20, 40, "f32s", "plain", "", ("planned", 3, 14, 18), "", "conv_core_kernel<f32s,3,4,2,4,2,3,0,1,1,0,0,0,1,-1>"),
    ("s1", 8, 72, "f32s", "bnadd", "src_out+stats", ("planned", 2, 26, 9), "", "conv_core_kernel<f32s,3,4,2,4,2,3,1,1,1,-1,1,0,0,-1>"),
    ("m24", 32, 8, "f32s", "bn", "bias+relu", ("planned", 8, 14, 18), "", "conv_core_kernel<f32s,3,8,1,2,2,3,0,0,3,-1,0,0,0,-1>"),
    ("m24b4", 4, 8, "f32s", "plain", "bias", ("planned", 8, 14, 18), "", "conv_core_kernel<f32s,3,8,1,2,2,3,0,0,4,1,0,0,0,-1>"),
    ("s1", 4, 8, "f32s", "bn", "bias+relu", ("planned", 8, 26, 9), "", "conv_core_kernel<f32s,3,8,1,2,2,3,0,0,4,1,0,0,0,48>"),
    ("tiny1", 32, 8, "f32s", "bn", "", ("planned", 8, 15, 2), "", "conv_core_kernel<f32s,3,8,1,2,2,3,0,1,4,-1,0,0,0,-1>"),
    ("m24", 4, 8, "f32s", "bn", "", ("planned", 8, 14, 18), "", "conv_core_kernel<f32s,3,8,1,2,2,3,0,1,4,1,0,0,0,-1>"),
    ("m24b4", 4, 8, "f32s", "bnadd_eval", "src_out", ("planned", 8, 14, 18), "", "conv_core_kernel<f32s,3,8,1,2,2,3,1,1,3,-1,1,0,0,-1>"),
    ("big", 128, 8, "f32s", "bn_relu", "bias+relu", ("planned", 1, 13, 37), "", "conv_core_kernel<f32s,3,8,1,4,2,6,0,0,1,-1,0,0,0,-1>"),
    ("big", 128, 8, "f32s", "bn", "relu+stats", ("planned", 1, 13, 37), "", "conv_core_kernel<f32s,3,8,1,4,2,6,0,1,1,-1,0,0,0,-1>"),
    ("m24", 128, 256, "bf16", "bn_relu_eval", "", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,1,0,0,0,2,4>"),
    ("m24b4", 32, 8, "bf16", "bn_relu", "", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,0,2,8>"),
    ("m24b4", 64, 40, "bf16", "bn_relu_eval", "", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,0,4,4>"),
    ("tiny1", 256, 256, "bf16", "plain", "bias+relu", ("planned", 6, 15, 2), "", "conv_r2_kernel<bf16,1,0,0,48,2,4>"),
    ("m24", 32, 8, "bf16", "bn_eval", "bias+relu", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,48,2,8>"),
    ("m24b4", 96, 72, "bf16", "plain", "bias+relu", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,48,4,4>"),
    ("s1", 128, 256, "bf16", "plain", "stats", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,1,0,0,8,2,4>"),
    ("tiny1", 32, 8, "bf16", "bn_relu_eval", "stats", ("forced", 10, 15, 2), "", "conv_r2_kernel<bf16,1,0,0,8,2,8>"),
    ("m24b4", 64, 40, "bf16", "plain", "stats", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,8,4,4>"),
    ("m24b4", 96, 72, "bf16", "bnbwd", "", ("planned", 6, 7, 18), "", "conv_r2_kernel<bf16,1,1,0,0,2,4>"),
    ("s1", 32, 8, "bf16", "bnbwd_eval", "", ("forced", 10, 26, 9), "", "conv_r2_kernel<bf16,1,1,0,0,2,8>"),
    ("tiny1", 96, 72, "bf16", "bnbwd_eval", "mask_y+red", ("planned", 6, 15, 2), "", "conv_r2_kernel<bf16,1,1,0,1,2,4>"),
    ("m24", 32, 8, "bf16", "bnbwd_eval", "mask_y+red", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,1,1,0,1,2,8>"),
    ("m24b4", 96, 72, "bf16", "bnbwd_eval", "addend", ("planned", 6, 7, 18), "", "conv_r2_kernel<bf16,1,1,0,2,2,4>"),
    ("s1", 32, 8, "bf16", "bnbwd", "addend", ("forced", 10, 26, 9), "", "conv_r2_kernel<bf16,1,1,0,2,2,8>"),
    ("tiny1", 64, 40, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 6, 15, 2), "", "conv_r2_kernel<bf16,1,1,0,7,2,4>"),
    ("m24", 32, 8, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,1,1,0,7,2,8>"),
    ("m24b4", 128, 256, "bf16", "bnadd", "src_out", ("planned", 6, 7, 18), "", "conv_r2_kernel<bf16,1,1,1,0,2,4>"),
    ("s1", 32, 8, "bf16", "bnadd_eval", "src_out", ("forced", 10, 26, 9), "", "conv_r2_kernel<bf16,1,1,1,0,2,8>"),
    ("m24", 64, 40, "bf16", "bnadd", "src_out", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,1,1,0,4,4>"),
    ("m24", 128, 256, "bf16", "bnadd_eval", "stats", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,1,1,1,8,2,4>"),
    ("m24b4", 32, 8, "bf16", "bnadd", "stats", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,1,1,1,8,2,8>"),
    ("m24", 96, 72, "bf16", "bnadd", "stats", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,1,1,8,4,4>"),
    ("tiny1", 96, 72, "mixed", "bnbwd", "", ("planned", 6, 15, 2), "", "conv_r2_kernel<bf16,2,1,0,0,2,4>"),
    ("m24", 32, 8, "mixed", "bnbwd", "", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,2,1,0,0,2,8>"),
    ("m24b4", 96, 72, "mixed", "bnbwd", "mask_y+red", ("planned", 6, 7, 18), "", "conv_r2_kernel<bf16,2,1,0,1,2,4>"),
    ("s1", 32, 8, "mixed", "bnbwd_eval", "mask_y+red", ("forced", 10, 26, 9), "", "conv_r2_kernel<bf16,2,1,0,1,2,8>"),
    ("tiny1", 96, 72, "mixed", "bnbwd_eval", "addend", ("planned", 6, 15, 2), "", "conv_r2_kernel<bf16,2,1,0,2,2,4>"),
    ("m24", 32, 8, "mixed", "bnbwd_eval", "addend", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,2,1,0,2,2,8>"),
    ("m24b4", 96, 72, "mixed", "bnbwd_eval", "mask_y+red+addend+mask_z", ("planned", 6, 7, 18), "", "conv_r2_kernel<bf16,2,1,0,7,2,4>"),
    ("s1", 32, 8, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 10, 26, 9), "", "conv_r2_kernel<bf16,2,1,0,7,2,8>"),
    ("tiny1", 128, 256, "f16", "plain", "", ("planned", 6, 15, 2), "", "conv_r2_kernel<f16,2,0,0,0,2,4>"),
    ("m24", 32, 8, "f16", "plain", "", ("forced", 10, 14, 18), "", "conv_r2_kernel<f16,2,0,0,0,2,8>"),
    ("s1", 64, 40, "f16", "bn_eval", "", ("planned", 5, 26, 9), "", "conv_r2_kernel<f16,2,0,0,0,4,4>"),
    ("s1", 128, 256, "f16", "bn", "bias+relu", ("planned", 6, 14, 9), "", "conv_r2_kernel<f16,2,0,0,48,2,4>"),
    ("tiny1", 32, 8, "f16", "bn", "bias+relu", ("forced", 10, 15, 2), "", "conv_r2_kernel<f16,2,0,0,48,2,8>"),
    ("s1", 64, 40, "f16", "bn_relu_eval", "bias+relu", ("planned", 5, 26, 9), "", "conv_r2_kernel<f16,2,0,0,48,4,4>"),
    ("m24b4", 128, 256, "f16", "bn", "stats", ("planned", 6, 7, 18), "", "conv_r2_kernel<f16,2,0,0,8,2,4>"),
    ("s1", 32, 8, "f16", "bn_relu", "stats", ("forced", 10, 26, 9), "", "conv_r2_kernel<f16,2,0,0,8,2,8>"),
    ("s1", 96, 72, "f16", "plain", "stats", ("planned", 5, 26, 9), "", "conv_r2_kernel<f16,2,0,0,8,4,4>"),
    ("m24", 256, 256, "f16", "bnadd", "src_out", ("planned", 6, 14, 9), "", "conv_r2_kernel<f16,2,1,1,0,2,4>"),
    ("m24b4", 32, 8, "f16", "bnadd", "src_out", ("forced", 10, 14, 18), "", "conv_r2_kernel<f16,2,1,1,0,2,8>"),
    ("s1", 64, 40, "f16", "bnadd", "src_out", ("planned", 5, 26, 9), "", "conv_r2_kernel<f16,2,1,1,0,4,4>"),
    ("tiny1", 128, 256, "f16", "bnadd_eval", "stats", ("planned", 6, 15, 2), "", "conv_r2_kernel<f16,2,1,1,8,2,4>"),
    ("m24", 32, 8, "f16", "bnadd_eval", "stats", ("forced", 10, 14, 18), "", "conv_r2_kernel<f16,2,1,1,8,2,8>"),
    ("s1", 64, 40, "f16", "bnadd", "stats", ("planned", 5, 26, 9), "", "conv_r2_kernel<f16,2,1,1,8,4,4>"),
    ("s1", 128, 256, "bf16", "bn", "", ("forced", 9, 14, 9), "", "conv_ws_kernel<bf16,3,2,2,3,0,1,-1>"),
    ("tiny1", 128, 256, "bf16", "bn_relu_eval", "stats", ("forced", 9, 15, 2), "", "conv_ws_kernel<bf16,3,2,2,3,0,1,8>"),
    ("m24", 256, 256, "bf16", "bnbwd", "mask_y+red+addend", ("forced", 9, 14, 9), "", "conv_ws_kernel<bf16,3,2,2,3,1,1,-1>"),
    ("m24b4", 128, 256, "bf16", "bnbwd", "", ("forced", 9, 7, 18), "", "conv_ws_kernel<bf16,3,2,2,3,1,1,0>"),
    ("s1", 128, 256, "bf16", "bnbwd_eval", "mask_y+red", ("forced", 9, 14, 9), "", "conv_ws_kernel<bf16,3,2,2,3,1,1,1>"),
    ("tiny1", 128, 256, "bf16", "bnbwd_eval", "addend", ("forced", 9, 15, 2), "", "conv_ws_kernel<bf16,3,2,2,3,1,1,2>"),
    ("m24", 128, 256, "bf16", "bnbwd_eval", "mask_y+red+addend+mask_z", ("forced", 9, 14, 9), "", "conv_ws_kernel<bf16,3,2,2,3,1,1,7>"),
    ("m24b4", 256, 256, "mixed", "bnbwd", "mask_z", ("forced", 9, 7, 18), "", "conv_ws_kernel<bf16,3,2,2,3,1,2,-1>"),
    ("s1", 256, 256, "mixed", "bnbwd", "", ("forced", 9, 14, 9), "", "conv_ws_kernel<bf16,3,2,2,3,1,2,0>"),
    ("tiny1", 256, 256, "mixed", "bnbwd", "mask_y+red", ("forced", 9, 15, 2), "", "conv_ws_kernel<bf16,3,2,2,3,1,2,1>"),
    ("m24", 256, 256, "mixed", "bnbwd", "addend", ("forced", 9, 14, 9), "", "conv_ws_kernel<bf16,3,2,2,3,1,2,2>"),
    ("m24b4", 256, 256, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 9, 7, 18), "", "conv_ws_kernel<bf16,3,2,2,3,1,2,7>"),
    ("tiny2", 8, 8, "bf16", "bn", "", ("planned", 7, 15, 2), "", "conv_ws_kernel<bf16,3,2,4,3,0,1,-1>"),
    ("tiny2", 24, 40, "bf16", "plain", "stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<bf16,3,2,4,3,0,1,8>"),
    ("wide2", 8, 8, "bf16", "plain", "bias+relu", ("planned", 7, 5, 22), "", "conv_ws_kernel<bf16,3,2,4,9,0,1,-1>"),
    ("s2b4", 8, 8, "bf16", "bn", "stats", ("planned", 7, 14, 9), "", "conv_ws_kernel<bf16,3,2,4,9,0,1,8>"),
    ("s1", 128, 256, "f16", "plain", "bias", ("forced", 9, 14, 9), "", "conv_ws_kernel<f16,3,2,2,3,0,2,-1>"),
    ("tiny1", 128, 256, "f16", "bn_relu", "stats", ("forced", 9, 15, 2), "", "conv_ws_kernel<f16,3,2,2,3,0,2,8>"),
    ("tiny2", 8, 8, "f16", "bn", "", ("planned", 7, 15, 2), "", "conv_ws_kernel<f16,3,2,4,3,0,2,-1>"),
    ("tiny2", 24, 40, "f16", "plain", "stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<f16,3,2,4,3,0,2,8>"),
    ("s2odd", 8, 8, "f16", "plain", "relu+stats", ("planned", 7, 15, 6), "", "conv_ws_kernel<f16,3,2,4,9,0,2,-1>"),
    ("s2even", 8, 8, "f16", "bn_eval", "stats", ("planned", 7, 14, 9), "", "conv_ws_kernel<f16,3,2,4,9,0,2,8>"),
    ("m24", 128, 256, "f32", "plain", "relu+stats", ("planned", 9, 14, 9), "", "conv_ws_kernel<f32,3,2,2,3,0,0,-1>"),
    ("m24b4", 128, 256, "f32", "bn_eval", "stats", ("planned", 9, 7, 18), "", "conv_ws_kernel<f32,3,2,2,3,0,0,8>"),
    ("s1", 256, 256, "f32", "bnbwd", "mask_y+red+addend", ("planned", 9, 14, 9), "", "conv_ws_kernel<f32,3,2,2,3,1,0,-1>"),
    ("tiny1", 256, 256, "f32", "bnbwd", "", ("planned", 9, 15, 2), "", "conv_ws_kernel<f32,3,2,2,3,1,0,0>"),
    ("m24", 256, 256, "f32", "bnbwd", "mask_y+red", ("planned", 9, 14, 9), "", "conv_ws_kernel<f32,3,2,2,3,1,0,1>"),
    ("m24b4", 256, 256, "f32", "bnbwd", "addend", ("planned", 9, 7, 18), "", "conv_ws_kernel<f32,3,2,2,3,1,0,2>"),
    ("s1", 256, 256, "f32", "bnbwd_eval", "mask_y+red+addend+mask_z", ("planned", 9, 14, 9), "", "conv_ws_kernel<f32,3,2,2,3,1,0,7>"),
    ("tiny2", 4, 8, "f32", "plain", "relu+stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<f32,3,2,4,3,0,0,-1>"),
    ("tiny2", 4, 8, "f32", "bn_relu_eval", "stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<f32,3,2,4,3,0,0,8>"),
    ("s2b4", 4, 8, "f32", "bn", "bias+relu", ("planned", 7, 14, 9), "", "conv_ws_kernel<f32,3,2,4,9,0,0,-1>"),
    ("s2odd", 4, 8, "f32", "plain", "stats", ("planned", 7, 15, 6), "", "conv_ws_kernel<f32,3,2,4,9,0,0,8>"),
    ("tiny1", 128, 256, "f32s", "plain", "", ("planned", 9, 15, 2), "", "conv_ws_kernel<f32s,3,2,2,3,0,0,-1>"),
    ("m24", 128, 256, "f32s", "plain", "stats", ("planned", 9, 14, 9), "", "conv_ws_kernel<f32s,3,2,2,3,0,0,8>"),
    ("tiny2", 4, 8, "f32s", "plain", "relu+stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<f32s,3,2,4,3,0,0,-1>"),
    ("tiny2", 4, 8, "f32s", "bn_relu_eval", "stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<f32s,3,2,4,3,0,0,8>"),
    ("s2even", 4, 8, "f32s", "plain", "bias+relu", ("planned", 7, 14, 9), "", "conv_ws_kernel<f32s,3,2,4,9,0,0,-1>"),
    ("wide2", 4, 8, "f32s", "bn", "stats", ("planned", 7, 5, 22), "", "conv_ws_kernel<f32s,3,2,4,9,0,0,8>"),
    ("s1", 48, 96, "bf16", "plain", "stats", ("planned", 3, 26, 9), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,1,1,0,0,1,1,-1>"),
    ("m24", 48, 96, "f16", "bn_relu", "stats", ("planned", 3, 14, 18), "", "conv_core_kernel<f16,3,4,2,4,2,3,0,1,1,0,0,2,1,-1>"),
    ("tiny1", 48, 96, "bf16", "bnadd", "src_out+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<bf16,3,4,1,2,4,3,1,1,1,-1,1,1,0,-1>"),
    ("m24", 48, 96, "bf16", "bnbwd", "mask_y+red", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,1>"),
    ("m24", 48, 96, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 3, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,2,1,7>"),
    ("s1", 256, 256, "bf16", "bn_relu", "stats", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,1,0,0,8,2,4>"),
    ("m24", 64, 64, "bf16", "bn_relu_eval", "stats", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,8,4,4>"),
    ("m24", 128, 64, "f16", "bn", "stats", ("planned", 5, 14, 18), "", "conv_r2_kernel<f16,2,0,0,8,4,4>"),
    ("m24b4", 64, 64, "bf16", "bn_relu", "bias+relu", ("planned", 5, 14, 18), "", "conv_r2_kernel<bf16,1,0,0,48,4,4>"),
    ("m24", 256, 256, "f16", "plain", "bias+relu", ("planned", 6, 14, 9), "", "conv_r2_kernel<f16,2,0,0,48,2,4>"),
    ("tiny1", 64, 64, "bf16", "bnadd", "src_out+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<bf16,3,4,1,2,4,3,1,1,1,-1,1,1,0,-1>"),
    ("tiny1", 128, 64, "f16", "bnadd", "src_out", ("planned", 0, 15, 2), "", "conv_core_kernel<f16,3,4,1,2,4,3,1,1,1,-1,1,2,0,-1>"),
    ("tiny1", 64, 64, "f32", "bnadd", "src_out+stats", ("planned", 0, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,4,3,1,1,1,-1,1,0,0,-1>"),
    ("tiny1", 32, 32, "bf16", "bnadd", "src_out+stats", ("planned", 8, 15, 2), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,1,3,-1,1,1,0,-1>"),
    ("tiny1", 32, 32, "f16", "bnadd_eval", "src_out", ("planned", 8, 15, 2), "", "conv_core_kernel<f16,3,8,1,2,2,3,1,1,3,-1,1,2,0,-1>"),
    ("m24", 256, 256, "bf16", "bnadd", "src_out+stats", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,1,1,1,8,2,4>"),
    ("tiny1", 64, 64, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 6, 15, 2), "", "conv_r2_kernel<bf16,2,1,0,7,2,4>"),
    ("tiny1", 64, 64, "f32", "bnbwd", "mask_y+red", ("planned", 0, 15, 2), "", "conv_core_kernel<f32,3,4,1,2,4,3,1,0,1,-1,0,0,0,-1>"),
    ("tiny1", 32, 32, "bf16", "bnbwd", "addend", ("planned", 8, 15, 2), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,2>"),
    ("m24", 32, 32, "bf16", "bn_relu", "stats", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,1,4,1,0,1,0,-1>"),
    ("m24", 32, 32, "f16", "bn_relu", "stats", ("planned", 8, 14, 18), "", "conv_core_kernel<f16,3,8,1,2,2,3,0,1,4,1,0,2,0,-1>"),
    ("m24", 32, 32, "mixed", "bnbwd", "mask_y+red", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,1>"),
    ("m24", 32, 32, "bf16", "bn_relu", "bias", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,0,4,1,0,1,0,-1>"),
    ("m24", 64, 64, "bf16", "bn_relu", "bias", ("planned", 5, 14, 18), "", "conv_core_kernel<bf16,3,4,2,4,2,3,0,0,1,0,0,1,1,-1>"),
    ("m24", 64, 64, "bf16", "bnbwd", "mask_z", ("planned", 6, 14, 9), "", "conv_core_kernel<bf16,3,4,1,2,4,3,1,0,1,-1,0,1,0,-1>"),
    ("wide2", 40, 72, "bf16", "bn_relu", "stats", ("planned", 7, 5, 16), "", "conv_ws_kernel<bf16,3,2,4,9,0,1,8>"),
    ("wide2", 20, 40, "f32", "plain", "stats", ("planned", 7, 5, 19), "", "conv_ws_kernel<f32,3,2,4,9,0,0,8>"),
    ("wide2", 8, 8, "f16", "bn", "", ("planned", 7, 5, 22), "", "conv_ws_kernel<f16,3,2,4,9,0,2,-1>"),
    ("s2odd", 64, 128, "bf16", "bn_relu", "stats", ("planned", 7, 15, 6), "", "conv_ws_kernel<bf16,3,2,4,9,0,1,8>"),
    ("s2even", 128, 64, "f16", "bn_relu_eval", "stats", ("planned", 7, 10, 9), "", "conv_ws_kernel<f16,3,2,4,9,0,2,8>"),
    ("tiny2", 48, 96, "bf16", "plain", "stats", ("planned", 7, 15, 2), "", "conv_ws_kernel<bf16,3,2,4,3,0,1,8>"),
    ("s2odd", 20, 72, "f32s", "bn_relu_eval", "", ("planned", 7, 15, 6), "", "conv_ws_kernel<f32s,3,2,4,9,0,0,-1>"),
    ("s2even", 64, 64, "f32", "bn", "bias+relu", ("planned", 7, 10, 9), "", "conv_ws_kernel<f32,3,2,4,9,0,0,-1>"),
    ("p1b", 96, 72, "bf16", "bn_relu", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,0,4,1,8,0>"),
    ("q24", 64, 128, "f16", "bn_relu", "stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f16,2,0,4,2,8,0>"),
    ("p1b", 256, 64, "f32", "plain", "", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,0,4,0,-1,0>"),
    ("p1b", 96, 72, "bf16", "bnadd", "src_out+stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,1,8,1>"),
    ("q24", 256, 64, "f16", "bnadd", "src_out", ("planned", -1, 0, 0), "", "conv1x1_kernel<f16,2,1,4,2,0,1>"),
    ("p1a", 128, 256, "f32", "bnadd_eval", "src_out+stats", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,1,4,0,8,1>"),
    ("p1b", 96, 72, "bf16", "bnbwd", "addend", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,1,2,0>"),
    ("q24", 64, 256, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", -1, 0, 0), "", "conv1x1_kernel<bf16,2,1,4,2,-1,0>"),
    ("p1a", 256, 64, "f32", "bnbwd", "mask_y+red", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32,2,1,4,0,-1,0>"),
    ("q24", 128, 64, "f32s", "bn_relu_eval", "bias", ("planned", -1, 0, 0), "", "conv1x1_kernel<f32s,2,0,4,0,-1,0>"),
    ("p1a", 48, 96, "bf16", "bn_relu", "stats", ("planned", 2, 26, 9), "", "conv_core_kernel<bf16,1,4,2,4,2,3,0,1,1,-1,0,1,0,-1>"),
    ("p1b", 24, 40, "f16", "plain", "bias+relu", ("planned", 2, 36, 7), "", "conv_core_kernel<f16,1,4,2,4,2,3,0,0,1,-1,0,2,0,-1>"),
    ("q24", 20, 40, "f32", "bnbwd", "addend", ("planned", 2, 25, 10), "", "conv_core_kernel<f32,1,4,2,4,2,3,1,0,1,-1,0,0,0,-1>"),
    ("p1a", 40, 72, "mixed", "bnbwd", "mask_y+red", ("planned", 2, 26, 9), "", "conv_core_kernel<bf16,1,4,2,4,2,3,1,0,1,-1,0,2,0,-1>"),
    ("m24b8", 8, 8, "bf16", "bn_relu", "stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,0,1,4,1,0,1,0,-1>"),
    ("m24b8", 8, 8, "bf16", "bnadd", "src_out+stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,1,1,3,-1,1,1,0,-1>"),
    ("m24b8", 32, 32, "bf16", "bn_relu", "stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,0,1,4,1,0,1,0,-1>"),
    ("m24b8", 32, 32, "bf16", "bnadd", "src_out+stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,1,1,3,-1,1,1,0,-1>"),
    ("m24b8", 24, 40, "bf16", "bn_relu", "stats", ("planned", 2, 14, 18), "8", "conv_core_kernel<bf16,3,4,2,4,2,3,0,1,1,-1,0,1,0,-1>"),
    ("m24b8", 40, 72, "bf16", "bn_relu", "stats", ("planned", 3, 14, 18), "8", "conv_core_kernel<bf16,3,4,2,4,2,3,0,1,1,0,0,1,1,-1>"),
    ("m24b8", 64, 64, "bf16", "bn_relu", "stats", ("planned", 5, 14, 18), "8", "conv_r2_kernel<bf16,1,0,0,8,4,4>"),
    ("m24b8", 64, 64, "bf16", "bnadd", "src_out+stats", ("planned", 5, 14, 18), "8", "conv_r2_kernel<bf16,1,1,1,8,4,4>"),
    ("m24b8", 128, 256, "bf16", "bn_relu", "stats", ("planned", 6, 7, 18), "8", "conv_r2_kernel<bf16,1,0,0,8,2,4>"),
    ("m24b8", 32, 32, "f16", "bn_relu", "stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<f16,3,8,1,2,2,3,0,1,4,1,0,2,0,-1>"),
    ("m24b8", 32, 32, "f16", "bnadd", "src_out+stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<f16,3,8,1,2,2,3,1,1,3,-1,1,2,0,-1>"),
    ("m24b8", 64, 64, "f16", "bn_relu", "stats", ("planned", 5, 14, 18), "8", "conv_r2_kernel<f16,2,0,0,8,4,4>"),
    ("m24b8", 64, 64, "f16", "bnadd", "src_out+stats", ("planned", 5, 14, 18), "8", "conv_r2_kernel<f16,2,1,1,8,4,4>"),
    ("m24b8", 4, 8, "f32", "bn_relu", "stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<f32,3,8,1,2,2,3,0,1,4,1,0,0,0,-1>"),
    ("m24b8", 4, 8, "f32", "bnadd", "src_out+stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<f32,3,8,1,2,2,3,1,1,3,-1,1,0,0,-1>"),
    ("m24b8", 64, 32, "f32", "bn_relu", "stats", ("planned", 8, 14, 18), "8", "conv_core_kernel<f32,3,8,1,2,2,3,0,1,4,-1,0,0,0,-1>"),
    ("m24b8", 20, 40, "f32", "bn_relu", "stats", ("planned", 3, 14, 18), "8", "conv_core_kernel<f32,3,4,2,4,2,3,0,1,1,0,0,0,1,-1>"),
    ("m24b8", 20, 40, "f32", "bnadd", "src_out+stats", ("planned", 3, 14, 18), "8", "conv_core_kernel<f32,3,4,2,4,2,3,1,1,1,-1,1,0,0,-1>"),
    ("m24b8", 128, 256, "f32", "bn_relu", "stats", ("planned", 9, 7, 18), "8", "conv_ws_kernel<f32,3,2,2,3,0,0,8>"),
    ("m24b8", 20, 40, "f32s", "bn_relu", "stats", ("planned", 3, 14, 18), "8", "conv_core_kernel<f32s,3,4,2,4,2,3,0,1,1,0,0,0,1,-1>"),
    ("m24b8", 8, 8, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,7>"),
    ("m24b8", 32, 32, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,7>"),
    ("m24b8", 40, 72, "bf16", "bnbwd", "mask_y+red+addend", ("planned", 3, 14, 18), "8", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,0,0,1,1,-1>"),
    ("m24b8", 64, 64, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 6, 7, 18), "8", "conv_r2_kernel<bf16,1,1,0,7,2,4>"),
    ("m24b8", 128, 256, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 6, 7, 18), "8", "conv_r2_kernel<bf16,1,1,0,7,2,4>"),
    ("m24b8", 32, 32, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 8, 14, 18), "8", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,7>"),
    ("m24b8", 64, 64, "mixed", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 6, 7, 18), "8", "conv_r2_kernel<bf16,2,1,0,7,2,4>"),
    ("m24b8", 4, 8, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 8, 14, 18), "8", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,4,1,0,0,0,7>"),
    ("m24b8", 20, 40, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 3, 14, 18), "8", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,7>"),
    ("m24b8", 128, 256, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 9, 7, 18), "8", "conv_ws_kernel<f32,3,2,2,3,1,0,7>"),
    ("q24b8", 96, 72, "bf16", "bn_relu", "stats", ("planned", -1, 0, 0), "8", "conv1x1_kernel<bf16,2,0,4,1,8,0>"),
    ("q24b8", 64, 128, "f32", "bnadd", "src_out+stats", ("planned", -1, 0, 0), "8", "conv1x1_kernel<f32,2,1,4,0,8,1>"),
    ("q24b8", 128, 64, "mixed", "bnbwd", "addend", ("planned", -1, 0, 0), "8", "conv1x1_kernel<bf16,2,1,4,2,2,0>"),
    ("q24b8", 64, 64, "bf16", "bnbwd", "mask_y+red", ("planned", -1, 0, 0), "8", "conv1x1_kernel<bf16,2,1,4,1,-1,0>"),
    ("q24b8", 24, 40, "f16", "bn", "stats", ("planned", 2, 42, 6), "8", "conv_core_kernel<f16,1,4,2,4,2,3,0,1,1,-1,0,2,0,-1>"),
    ("s2b16", 24, 40, "bf16", "bn_relu", "stats", ("planned", 7, 14, 9), "8", "conv_ws_kernel<bf16,3,2,4,9,0,1,8>"),
    ("s2b16", 20, 72, "f32", "plain", "stats", ("planned", 7, 10, 9), "8", "conv_ws_kernel<f32,3,2,4,9,0,0,8>"),
    ("s2b16", 64, 64, "f16", "bn_relu", "", ("planned", 7, 10, 9), "8", "conv_ws_kernel<f16,3,2,4,9,0,2,-1>"),
    ("m24", 32, 32, "bf16", "bn_relu", "bias", ("forced", 10, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,0,0,4,1,0,1,0,-1>"),
    ("m24", 32, 32, "mixed", "bnbwd", "mask_z", ("forced", 10, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,-1>"),
    ("tiny1", 32, 32, "f16", "bnadd", "src_out+stats", ("forced", 10, 15, 2), "", "conv_r2_kernel<f16,2,1,1,8,2,8>"),
    ("m24b4", 32, 32, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("forced", 10, 14, 18), "", "conv_r2_kernel<bf16,1,1,0,7,2,8>"),
    ("m24b4", 32, 32, "f16", "bn_relu", "stats", ("forced", 10, 14, 18), "", "conv_r2_kernel<f16,2,0,0,8,2,8>"),
    ("u13", 32, 32, "bf16", "bnbwd", "mask_y+red", ("planned", 8, 23, 11), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,1,0,1>"),
    ("u24", 32, 32, "mixed", "bnbwd", "addend", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,4,1,0,2,0,2>"),
    ("u13", 64, 32, "bf16", "bnbwd", "", ("planned", 8, 23, 11), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,3,-1,0,1,0,-1>"),
    ("u24", 64, 32, "mixed", "bnbwd", "mask_y+red+addend", ("planned", 8, 14, 18), "", "conv_core_kernel<bf16,3,8,1,2,2,3,1,0,3,-1,0,2,0,-1>"),
    ("u13", 64, 64, "bf16", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 6, 11, 11), "", "conv_r2_kernel<bf16,1,1,0,7,2,4>"),
    ("u24", 128, 64, "mixed", "bnbwd", "mask_y+red", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,2,1,0,1,2,4>"),
    ("u24", 64, 128, "bf16", "bnbwd", "addend", ("planned", 6, 14, 9), "", "conv_r2_kernel<bf16,1,1,0,2,2,4>"),
    ("u13", 64, 64, "mixed", "bnbwd", "", ("planned", 6, 11, 11), "", "conv_r2_kernel<bf16,2,1,0,0,2,4>"),
    ("u13", 24, 40, "bf16", "bnbwd", "mask_y+red", ("planned", 2, 23, 11), "", "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,-1,0,1,0,-1>"),
    ("u13", 20, 40, "f32", "bnbwd", "mask_y+red", ("planned", 3, 23, 11), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,1>"),
    ("u24", 64, 64, "f32", "bnbwd", "mask_y+red+addend+mask_z", ("planned", 3, 14, 18), "", "conv_core_kernel<f32,3,4,2,4,2,3,1,0,1,0,0,0,1,7>"),
    ("u24", 32, 8, "f32", "bnbwd", "", ("planned", 8, 14, 18), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,3,-1,0,0,0,-1>"),
    ("u13", 64, 32, "f32", "bnbwd", "addend", ("planned", 8, 23, 11), "", "conv_core_kernel<f32,3,8,1,2,2,3,1,0,3,-1,0,0,0,-1>"),
    ("m24b8", 32, 32, "bf16", "bn_relu", "stats", ("forced", 10, 14, 18), "8", "conv_r2_kernel<bf16,1,0,0,8,2,8>"),
    ("m24b8", 32, 32, "mixed", "bnbwd", "mask_y+red", ("forced", 10, 14, 18), "8", "conv_r2_kernel<bf16,2,1,0,1,2,8>"),
]

# (.., the text the error must contain): launches stl_conv_forward refuses on the host
REFUSED = [
    ("m24", 24, 40, "bf16", "plain", "", ("forced", 2, 1, 256), "", "too large a halo"),       # 3 x 258 halo: 7 vectors per thread > 3
    ("m24", 8, 8, "f16", "bn", "", ("forced", 8, 2, 128), "", "too large a halo"),
    ("wide2", 20, 40, "f32", "plain", "", ("forced", 7, 2, 64), "", "too large a halo"),        # stride 2: 5 x 129 halo, 11 > 9
    ("s1", 24, 40, "bf16", "plain", "", ("forced", 0, 16, 16), "", "exceeds block shape"),
    ("s1", 4, 8, "f32", "plain", "", ("tile128", -1, 16, 9), "", "exceeds 128 pixels"),
    ("s1", 24, 40, "mixed", "plain", "", ("planned", 2, 26, 9), "", "not a data gradient"),    # ydtype on a forward launch
    ("p1a", 64, 64, "mixed", "bn_relu", "stats", ("planned", -1, 0, 0), "", "not a data gradient"),
    ("s1", 24, 40, "f16", "bnbwd", "", ("planned", 2, 26, 9), "", "forward-tensor type"),        # gradients are bf16
    ("s1", 20, 40, "f32s", "bnbwd", "", ("planned", 3, 26, 9), "", "STL_MATH_BF16X3"),
    ("s1", 128, 256, "f32", "bnadd", "src_out", ("planned", 9, 14, 9), "", "no block-end"),      # no BNADD form of the wave-specialised kernel
    ("s2odd", 24, 40, "bf16", "bnadd", "src_out", ("planned", 7, 15, 6), "", "a BNADD source needs"),
    ("s1", 24, 40, "bf16", "bnadd", "src_out+bias", ("planned", 2, 26, 9), "", "takes no epilogue operands"),
]

# Instantiations the dispatch can reach when a caller forces a block shape, but that no planner setting emits for any
# descriptor (1x1 convolutions on the C <= 32 blocks, shapes 4 and 8, and on the wave-specialised blocks; data gradients on the
# 512-pixel block and on the stride-2 block, shape 7): compiled, not planned, not launched by these tests.
NOT_PLANNED = [
    "conv_core_kernel<bf16,1,4,1,2,2,3,0,0,4,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,0,0,4,1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,0,1,4,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,0,1,4,1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,1,0,3,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,1,0,3,-1,0,2,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,1,0,4,1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,4,1,2,2,3,1,0,4,1,0,2,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,0,0,4,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,0,0,4,1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,0,1,4,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,0,1,4,1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,1,0,3,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,1,0,3,-1,0,2,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,1,0,4,1,0,1,0,-1>",
    "conv_core_kernel<bf16,1,8,1,2,2,3,1,0,4,1,0,2,0,-1>",
    "conv_core_kernel<bf16,3,8,1,4,2,6,1,0,1,-1,0,1,0,-1>",
    "conv_core_kernel<bf16,3,8,1,4,2,6,1,0,1,-1,0,2,0,-1>",
    "conv_core_kernel<f16,1,4,1,2,2,3,0,0,4,-1,0,2,0,-1>",
    "conv_core_kernel<f16,1,4,1,2,2,3,0,0,4,1,0,2,0,-1>",
    "conv_core_kernel<f16,1,4,1,2,2,3,0,1,4,-1,0,2,0,-1>",
    "conv_core_kernel<f16,1,4,1,2,2,3,0,1,4,1,0,2,0,-1>",
    "conv_core_kernel<f16,1,8,1,2,2,3,0,0,4,-1,0,2,0,-1>",
    "conv_core_kernel<f16,1,8,1,2,2,3,0,0,4,1,0,2,0,-1>",
    "conv_core_kernel<f16,1,8,1,2,2,3,0,1,4,-1,0,2,0,-1>",
    "conv_core_kernel<f16,1,8,1,2,2,3,0,1,4,1,0,2,0,-1>",
    "conv_core_kernel<f32,1,4,1,2,2,3,0,0,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32,1,4,1,2,2,3,0,0,4,1,0,0,0,-1>",
    "conv_core_kernel<f32,1,4,1,2,2,3,0,1,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32,1,4,1,2,2,3,0,1,4,1,0,0,0,-1>",
    "conv_core_kernel<f32,1,4,1,2,2,3,1,0,3,-1,0,0,0,-1>",
    "conv_core_kernel<f32,1,4,1,2,2,3,1,0,4,1,0,0,0,-1>",
    "conv_core_kernel<f32,1,8,1,2,2,3,0,0,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32,1,8,1,2,2,3,0,0,4,1,0,0,0,-1>",
    "conv_core_kernel<f32,1,8,1,2,2,3,0,1,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32,1,8,1,2,2,3,0,1,4,1,0,0,0,-1>",
    "conv_core_kernel<f32,1,8,1,2,2,3,1,0,3,-1,0,0,0,-1>",
    "conv_core_kernel<f32,1,8,1,2,2,3,1,0,4,1,0,0,0,-1>",
    "conv_core_kernel<f32,3,8,1,4,2,6,1,0,1,-1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,4,1,2,2,3,0,0,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,4,1,2,2,3,0,0,4,1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,4,1,2,2,3,0,1,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,4,1,2,2,3,0,1,4,1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,8,1,2,2,3,0,0,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,8,1,2,2,3,0,0,4,1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,8,1,2,2,3,0,1,4,-1,0,0,0,-1>",
    "conv_core_kernel<f32s,1,8,1,2,2,3,0,1,4,1,0,0,0,-1>",
    "conv_ws_kernel<bf16,1,2,2,3,0,1,-1>",
    "conv_ws_kernel<bf16,1,2,2,3,1,1,-1>",
    "conv_ws_kernel<bf16,1,2,2,3,1,2,-1>",
    "conv_ws_kernel<bf16,1,2,4,3,0,1,-1>",
    "conv_ws_kernel<bf16,1,2,4,3,1,1,-1>",
    "conv_ws_kernel<bf16,1,2,4,3,1,2,-1>",
    "conv_ws_kernel<bf16,3,2,4,3,1,1,-1>",
    "conv_ws_kernel<bf16,3,2,4,3,1,2,-1>",
    "conv_ws_kernel<bf16,3,2,4,9,1,1,-1>",
    "conv_ws_kernel<bf16,3,2,4,9,1,2,-1>",
    "conv_ws_kernel<f16,1,2,2,3,0,2,-1>",
    "conv_ws_kernel<f16,1,2,4,3,0,2,-1>",
    "conv_ws_kernel<f32,1,2,2,3,0,0,-1>",
    "conv_ws_kernel<f32,1,2,2,3,1,0,-1>",
    "conv_ws_kernel<f32,1,2,4,3,0,0,-1>",
    "conv_ws_kernel<f32,1,2,4,3,1,0,-1>",
    "conv_ws_kernel<f32,3,2,4,3,1,0,-1>",
    "conv_ws_kernel<f32,3,2,4,9,1,0,-1>",
    "conv_ws_kernel<f32s,1,2,2,3,0,0,-1>",
    "conv_ws_kernel<f32s,1,2,4,3,0,0,-1>",
]
