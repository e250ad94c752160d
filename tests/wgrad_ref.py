"""Plain fp64 CPU references, case tables and error bound for the weight-gradient kernels (wgrad.hip) and the stride-2 data
gradient (the zero-stuffed source of conv_core.hip).  Shared by tests/test_wgrad_exact_gpu.py (which runs the kernels) and
tests/test_wgrad_ref_cpu.py (which checks this file against float64 autograd, the bound against an emulation, and the case
tables against the dispatch rules of wgrad.hip, restated below)."""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
INT_VALUES = (-3, -2, -1, 1, 2, 3)   # exact in bf16, f16 and fp32; every product and every partial sum below 2^24 is exact
MAX_EXACT_PIXELS = 4096              # |dw| <= 9 * B * Ho * Wo < 2^24
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# dt -> (T: gradient tensors and MFMA operands, TY: stored forward tensors h.x / g.y)
TYPES = {"fp32": ("f32", "f32"), "bf16": ("bf16", "bf16"), "mixed": ("bf16", "f16")}
U_T = {"f32": 0.0, "bf16": 2.0 ** -8}

# name: (B, Hi, Wi, ks, stride)
GEOMS = {
    "s1": (2, 12, 9, 3, 1),        # 3x3 stride 1, odd width
    "s2odd": (3, 13, 11, 3, 2),    # 3x3 stride 2, odd sizes -> 7x6
    "s2even": (2, 24, 18, 3, 2),   # 3x3 stride 2, even sizes -> 12x9
    "p1a": (2, 12, 9, 1, 1),       # 1x1 stride 1
    "p1b": (3, 11, 7, 1, 1),
    "p2": (2, 13, 11, 1, 2),       # 1x1 stride 2 -> 7x6: the way into the 1x1 kernel's large-halo buckets
    "p2big": (2, 15, 31, 1, 2),    # ... -> 8x16, so that an 8x16 tile is full of pixels
    "tiny1": (5, 2, 2, 3, 1),      # 2x2 maps: a tall tile spans three or more images across their separator rows
    "tiny2": (5, 4, 4, 3, 2),      # 4x4 -> 2x2 at stride 2 (PI = 6 > Hi)
    "wide2": (1, 7, 255, 3, 2),    # -> 4x128: fills the 2x64 and 1x128 tiles of the largest bf16 halo bucket
}
CHANNELS = [(8, 8), (32, 32), (48, 40), (64, 64), (128, 64), (96, 72), (16, 96)]   # (Ci, Co)


def out_hw(geom):
    B, Hi, Wi, ks, s = GEOMS[geom]
    pad = 1 if ks == 3 else 0
    return (Hi + 2 * pad - ks) // s + 1, (Wi + 2 * pad - ks) // s + 1


# ------------------------------------------------------------------------------------------------ references
def wgrad_fp64(h, g, ks, stride):
    """dw[co][tap][ci] = sum_pixels g[pixel][co] * h[pixel * stride + tap - pad][ci] in float64 on the CPU.
    h: [B, Hi, Wi, Ci], g: [B, Ho, Wo, Co] (NHWC, any dtype).  Returns the kernel's slab layout [Co][ks * ks][Ci]."""
    x = h.detach().cpu().double().permute(0, 3, 1, 2).contiguous()
    go = g.detach().cpu().double().permute(0, 3, 1, 2).contiguous()
    Co, Ci = go.shape[1], x.shape[1]
    dw = torch.nn.grad.conv2d_weight(x, (Co, Ci, ks, ks), go, stride=stride, padding=1 if ks == 3 else 0)
    return dw.permute(0, 2, 3, 1).reshape(Co, ks * ks, Ci).contiguous()


def dgrad_fp64(g, w, H, W):
    """Data gradient of a 3x3 stride-2 convolution in float64 on the CPU.  g: [B, Ho, Wo, Co] NHWC, w: [Co][3][3][Ci] (the
    forward weights, NHWC).  Returns [B, H, W, Ci]."""
    go = g.detach().cpu().double().permute(0, 3, 1, 2).contiguous()
    wt = w.detach().cpu().double().permute(0, 3, 1, 2).contiguous()   # [Co][Ci][3][3] = conv_transpose2d's (in, out, kh, kw)
    Ho, Wo = go.shape[2:]
    op = (H - (2 * (Ho - 1) + 1), W - (2 * (Wo - 1) + 1))
    dx = F.conv_transpose2d(go, wt, stride=2, padding=1, output_padding=op)
    assert dx.shape[2:] == (H, W)
    return dx.permute(0, 2, 3, 1).contiguous()


def int_tensor(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(INT_VALUES, dtype=torch.float64)[torch.randint(0, len(INT_VALUES), shape, generator=g)]


@functools.lru_cache(maxsize=None)
def exact_problem(geom, Ci, Co):
    """Integer h, g and the fp64 weight gradient of one geometry (shared by every dtype, tile and split: never modified)."""
    B, Hi, Wi, ks, s = GEOMS[geom]
    Ho, Wo = out_hw(geom)
    assert B * Ho * Wo <= MAX_EXACT_PIXELS
    h = int_tensor((B, Hi, Wi, Ci), 1000 + 7 * Ci + Co)
    g = int_tensor((B, Ho, Wo, Co), 2000 + 7 * Ci + Co)
    return h, g, wgrad_fp64(h, g, ks, s)


# ------------------------------------------------------------------------------------------------ dispatch rules, restated
def ceil_div(a, b):
    return -(-a // b)


def halo_pixels(ks, stride, TH, TW):
    return ((TH - 1) * stride + ks) * ((TW - 1) * stride + ks)


def tiles_per_problem(geom, TH, TW):
    B = GEOMS[geom][0]
    Ho, Wo = out_hw(geom)
    return ceil_div(B * (Ho + 1), TH) * ceil_div(Wo, TW)


def _bucket(n, sizes):
    return next((s for s in sizes if n <= s), None)


def family(dt, ks, stride, Ci, Co):
    """Which kernel serves a problem: 'c64' (wgrad_kernel, 16 waves, 64-channel blocks), 'wide' (wgrad64_kernel) or '32'."""
    if TYPES[dt][0] == "bf16" and stride == 1 and Ci >= 64 and Co >= 64:
        return "c64" if ks == 3 else "wide"
    return "32"


def instantiation(dt, ks, stride, Ci, Co, TH, TW, gq):
    """(kernel, T, KS, NVH, GQ, NW, TY, CH) that stl_conv_wgrad launches, or None where it refuses the tile (halo too large).
    Restates wgrad_c64_3x3 / wgrad_chunk / dispatch / dispatch64 of wgrad.hip."""
    T, TY = TYPES[dt]
    hp, gq = halo_pixels(ks, stride, TH, TW), int(bool(gq))
    assert TH * TW <= 128
    fam = family(dt, ks, stride, Ci, Co)
    if fam == "c64":       # 1024 threads, 8 vectors of 8 channels per pixel
        nvh = _bucket(ceil_div(hp * 8, 1024), (2, 3))
        return None if nvh is None else ("wgrad_kernel", T, 3, nvh, gq, 16, TY, 64)
    if fam == "wide":      # 256 threads; stride 1, so the halo is the tile: at most 128 * 8 / 256 = 4 vectors
        assert ceil_div(hp * 8, 256) <= 6
        return ("wgrad64_kernel", T, 1, 6, gq, 4, TY, 64)
    vpx = 8 if T == "f32" else 4   # 16-byte vectors per pixel of 32 channels
    if ks == 3:
        nvh, nw = _bucket(ceil_div(hp * vpx, 512), (2, 3, 5, 9)), 8
    else:
        nvh, nw = _bucket(ceil_div(hp * vpx, 256), (3, 6, 9, 18)), 4
    return None if nvh is None else ("wgrad_kernel", T, ks, nvh, gq, nw, TY, 32)


def reachable_instantiations():
    """Everything dispatch(), dispatch64() and the 64-channel path can return: every tile of at most 128 pixels, both
    strides, both kernel sizes, both channel classes, every type pair.  (wgrad_kernel<bf16, 1, 18, ...> is compiled but no tile
    reaches it: a 1x1 stride-2 halo is (2 TH - 1)(2 TW - 1) <= 465 pixels = 8 vectors per thread.)"""
    out = set()
    for dt in TYPES:
        for ks in (1, 3):
            for stride in (1, 2):
                for C in (32, 64):
                    for TH in range(1, 129):
                        for TW in range(1, 128 // TH + 1):
                            for gq in (0, 1):
                                out.add(instantiation(dt, ks, stride, C, C, TH, TW, gq))
    out.discard(None)
    return out


_CODE = {"0": "f32", "1": "bf16", "2": "f16"}   # STL_F32 / STL_BF16 / STL_F16


def parse_kernel_name(name):
    """stl_last_kernel() -> the tuple of instantiation()."""
    base, args = name.rstrip(">").split("<")
    a = args.split(",")
    if base == "wgrad_kernel":     # <T, KS, NVH, GQ, TPX, OCC, NW, TY, CH>
        return (base, a[0], int(a[1]), int(a[2]), int(a[3]), int(a[6]), _CODE[a[7]], int(a[8]))
    assert base == "wgrad64_kernel", name   # <T, KS, NVH, GQ, TPX, TY>: 4 waves, 64-channel blocks
    return (base, a[0], int(a[1]), int(a[2]), int(a[3]), 4, _CODE[a[5]], 64)


# ------------------------------------------------------------------------------------------------ case tables
# (geometry, TH, TW, tiles, NVH the tile lands in: f32 / bf16 32-channel blocks, and "c64" the 64-channel 3x3 blocks; None = the
# launch is refused).  The wide 1x1 kernel has one bucket (6).  tests/test_wgrad_ref_cpu.py checks every figure against the rules.
TILES = [
    ("s1", 4, 9, 7, {"f32": 2, "bf16": 2, "c64": 2}),        # odd tile count >= 5
    ("s1", 5, 4, 18, {"f32": 2, "bf16": 2, "c64": 2}),       # divides neither Wo nor B (Ho + 1)
    ("s1", 8, 16, 4, {"f32": 3, "bf16": 2, "c64": 2}),
    ("s1", 2, 64, 13, {"f32": 5, "bf16": 3, "c64": 3}),
    ("s1", 1, 128, 26, {"f32": 9, "bf16": 5, "c64": None}),  # one pixel high; halo 390: refused by the 64-channel kernel
    ("s1", 128, 1, 9, {"f32": 9, "bf16": 5, "c64": None}),   # one pixel wide
    ("s1", 13, 9, 2, {"f32": 3, "bf16": 2, "c64": 2}),
    ("s1", 26, 4, 3, {"f32": 3, "bf16": 2, "c64": 2}),
    ("s2odd", 3, 4, 16, {"f32": 2, "bf16": 2}),
    ("s2odd", 5, 5, 10, {"f32": 2, "bf16": 2}),
    ("s2odd", 4, 10, 6, {"f32": 3, "bf16": 2}),
    ("s2odd", 8, 6, 3, {"f32": 5, "bf16": 2}),
    ("s2odd", 4, 16, 6, {"f32": 5, "bf16": 3}),
    ("s2odd", 8, 16, 3, {"f32": 9, "bf16": 5}),
    ("s2odd", 24, 5, 2, {"f32": 9, "bf16": 5}),
    ("s2odd", 2, 64, 12, {"f32": None, "bf16": 9}),
    ("s2even", 4, 9, 7, {"f32": 3, "bf16": 2}),
    ("s2even", 7, 4, 12, {"f32": 3, "bf16": 2}),
    ("s2even", 13, 9, 2, {"f32": 9, "bf16": 5}),
    ("s2even", 5, 16, 6, {"f32": 9, "bf16": 3}),
    ("s2even", 1, 128, 26, {"f32": None, "bf16": 9}),
    ("wide2", 2, 64, 6, {"f32": None, "bf16": 9}),           # halo 5 x 129 = 645, every pixel of it inside the map
    ("wide2", 1, 128, 5, {"f32": None, "bf16": 9}),
    ("wide2", 4, 30, 10, {"f32": 9, "bf16": 5}),
    ("tiny1", 8, 2, 2, {"f32": 2, "bf16": 2, "c64": 2}),     # one tile = images 0, 1 and most of 2
    ("tiny1", 16, 2, 1, {"f32": 2, "bf16": 2, "c64": 2}),    # one tile = the whole batch and a row beyond it
    ("tiny1", 9, 1, 4, {"f32": 2, "bf16": 2, "c64": 2}),
    ("tiny2", 8, 2, 2, {"f32": 2, "bf16": 2}),
    ("tiny2", 16, 2, 1, {"f32": 3, "bf16": 2}),
    ("tiny2", 8, 3, 2, {"f32": 2, "bf16": 2}),
    ("tiny2", 5, 2, 3, {"f32": 2, "bf16": 2}),
    ("p1a", 4, 9, 7, {"f32": 3, "bf16": 3}),
    ("p1a", 13, 9, 2, {"f32": 6, "bf16": 3}),
    ("p1a", 5, 4, 18, {"f32": 3, "bf16": 3}),
    ("p1a", 1, 128, 26, {"f32": 6, "bf16": 3}),
    ("p1a", 128, 1, 9, {"f32": 6, "bf16": 3}),
    ("p1b", 6, 7, 6, {"f32": 3, "bf16": 3}),
    ("p1b", 5, 3, 24, {"f32": 3, "bf16": 3}),
    ("p1b", 16, 8, 3, {"f32": 6, "bf16": 3}),
    ("p2", 4, 6, 4, {"f32": 3, "bf16": 3}),
    ("p2", 8, 6, 2, {"f32": 6, "bf16": 3}),
    ("p2", 3, 4, 12, {"f32": 3, "bf16": 3}),
    ("p2", 4, 16, 4, {"f32": 9, "bf16": 6}),
    ("p2", 8, 16, 2, {"f32": 18, "bf16": 9}),
    ("p2big", 8, 16, 3, {"f32": 18, "bf16": 9}),
    ("p2big", 4, 16, 5, {"f32": 9, "bf16": 6}),
    ("p2big", 9, 7, 6, {"f32": 9, "bf16": 6}),
]


def stated_instantiation(row, dt, Ci, Co, gq):
    """The instantiation a case expects, from what its TILES row states (None: the row states a refusal)."""
    geom, TH, TW, npt, nvh = row
    ks, stride = GEOMS[geom][3:]
    T, TY = TYPES[dt]
    fam = family(dt, ks, stride, Ci, Co)
    if fam == "wide":
        return ("wgrad64_kernel", T, 1, 6, int(gq), 4, TY, 64)
    n = nvh["c64" if fam == "c64" else T]
    if n is None:
        return None
    return ("wgrad_kernel", T, ks, n, int(gq), 16 if fam == "c64" else (8 if ks == 3 else 4), TY, 64 if fam == "c64" else 32)


def _splits(npt):
    return sorted({1, min(2, npt), npt})


def exact_cases():
    """(row, dt, Ci, Co, nsplit) of section 1: every tile with every type and nsplit in {1, 2, tiles}; the channel pairs rotate
    so that each meets every type, kernel size and stride.  Tiles the 32-channel kernel refuses appear in refused_cases()."""
    out = []
    for r, row in enumerate(TILES):
        for d, dt in enumerate(TYPES):
            for s, ns in enumerate(_splits(row[3])):
                Ci, Co = CHANNELS[(r + d + s) % len(CHANNELS)]
                if stated_instantiation(row, dt, Ci, Co, 0) is None:
                    Ci, Co = 32, 32   # the 64-channel kernel refuses this tile: run the 32-channel one
                if stated_instantiation(row, dt, Ci, Co, 0) is not None:
                    out.append((row, dt, Ci, Co, ns))
    return out


def refused_cases():
    """(row, dt, Ci, Co): launches that must return the 'halo ... too large' error without running anything."""
    out = [(row, "bf16", 64, 64) for row in TILES if row[4].get("c64", 0) is None]
    out += [(row, "fp32", 32, 32) for row in TILES if row[4]["f32"] is None]
    return out


H_MODES = ("bn_relu", "bn", "bn_eval", "plain")


def xform_cases():
    """(row, dt, Ci, Co, nsplit, hmode, gmode) of section 3.  Every tile and type with a BNBWD gradient source (the GQ
    instantiations), the h mode rotating; and per geometry one tile with a PLAIN gradient beside each BN form of h."""
    out = []
    for r, row in enumerate(TILES):
        for d, dt in enumerate(TYPES):
            Ci, Co = CHANNELS[(r + 2 * d + 1) % len(CHANNELS)]
            if stated_instantiation(row, dt, Ci, Co, 1) is None:
                Ci, Co = 32, 32
            if stated_instantiation(row, dt, Ci, Co, 1) is None:
                continue
            out.append((row, dt, Ci, Co, min(2, row[3]), H_MODES[(r + d) % 4], "bnbwd"))
            ks, stride = GEOMS[row[0]][3:]
            if family(dt, ks, stride, 64, 64) != family(dt, ks, stride, Ci, Co) and row[4].get("c64", 6) is not None:
                Ci, Co = CHANNELS[3 + (r + d) % 3]   # the 64-channel kernels (3x3 blocks of 16 waves, wide 1x1) on the same tile
                out.append((row, dt, Ci, Co, min(3, row[3]), H_MODES[(r + d + 1) % 4], "bnbwd"))
    seen = set()
    for r, row in enumerate(TILES):
        if row[0] in seen or row[4]["f32"] is None:
            continue
        seen.add(row[0])
        for d, dt in enumerate(TYPES):
            for m, hmode in enumerate(H_MODES[:3]):
                Ci, Co = CHANNELS[(r + d + m + 2) % len(CHANNELS)]
                out.append((row, dt, Ci, Co, min(3, row[3]), hmode, "plain"))
    return out


def case_id(case):
    row, dt, Ci, Co = case[:4]
    return "-".join([row[0], f"{row[1]}x{row[2]}", dt, f"{Ci}x{Co}"] + [str(v) for v in case[4:]])


# ------------------------------------------------------------------------------------------------ transformed sources
def spread(n, lo, hi, gen):
    """n values log-uniform in [lo, hi] (hi / lo >= 4): clearly different from channel to channel."""
    return torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(hi / lo)) * lo


@functools.lru_cache(maxsize=None)
def xform_problem(geom, Ci, Co, dt):
    """Real-valued stored tensors and BatchNorm parameters of one geometry and type (never modified).
    x: h as stored (TY), y: the conv output as stored (TY), dy: the gradient dt as stored (T).  Channel c of x has mean mu[c]
    and deviation sd[c], each drawn over a 4x range or more, and so have gamma, beta and the running statistics."""
    B, Hi, Wi, ks, s = GEOMS[geom]
    Ho, Wo = out_hw(geom)
    T, TY = TYPES[dt]
    gen = torch.Generator().manual_seed(31 * Ci + Co + 5)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    sign = lambda n: torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    P = {}
    P["x"] = (rnd(B, Hi, Wi, Ci) * spread(Ci, 0.5, 2.0, gen) + spread(Ci, 0.25, 1.0, gen) * sign(Ci)).to(TORCH_DT[TY])
    P["y"] = (rnd(B, Ho, Wo, Co) * spread(Co, 0.5, 2.0, gen) + spread(Co, 0.25, 1.0, gen) * sign(Co)).to(TORCH_DT[TY])
    P["dy"] = (rnd(B, Ho, Wo, Co) * spread(Co, 0.5, 2.0, gen)).to(TORCH_DT[T])
    P["gamma_h"], P["beta_h"] = spread(Ci, 0.5, 2.0, gen).float(), (spread(Ci, 0.25, 1.0, gen) * sign(Ci)).float()
    P["rmean_h"], P["rvar_h"] = (spread(Ci, 0.25, 1.0, gen) * sign(Ci)).float(), spread(Ci, 0.25, 4.0, gen).float()
    P["gamma_g"] = spread(Co, 0.5, 2.0, gen).float()
    return P


def channel_stats(t):
    """[2][C] fp64: per-channel sum and sum of squares of a stored tensor."""
    f = t.double().reshape(-1, t.shape[-1])
    return torch.stack([f.sum(0), (f * f).sum(0)])


def h_constants(P, hmode):
    """fp64 (a, b) of h' = a x + b from the STORED x (batch statistics) or the running statistics (eval)."""
    gamma, beta = P["gamma_h"].double(), P["beta_h"].double()
    if hmode == "bn_eval":
        mean, var = P["rmean_h"].double(), P["rvar_h"].double()
    else:
        f = P["x"].double().reshape(-1, P["x"].shape[-1])
        mean, var = f.mean(0), f.var(0, unbiased=False)
    a = gamma / torch.sqrt(var + EPS)
    return a, beta - mean * a


def g_constants(P):
    """fp64 (a, b, c_mean, c_sum, r) of BatchNorm backward on load, g' = a dy + b y + c_mean + c_sum, from the stored y, dy.
    r: the [2][Co] reductions (sum dy, sum dy * yhat) that the kernel reads as rstats."""
    y, dy = P["y"].double().reshape(-1, P["y"].shape[-1]), P["dy"].double().reshape(-1, P["y"].shape[-1])
    mean, rstd = y.mean(0), 1.0 / torch.sqrt(y.var(0, unbiased=False) + EPS)
    r = torch.stack([dy.sum(0), (dy * (y - mean) * rstd).sum(0)])
    c1, c2 = r[0] / y.shape[0], r[1] / y.shape[0]
    al = P["gamma_g"].double() * rstd
    return al, -al * rstd * c2, al * mean * rstd * c2, -al * c1, r


def transformed(P, hmode, gmode, hconst=None, gconst=None):
    """fp64 operands of the weight gradient and their magnitude tensors (every term of the transform replaced by its
    absolute value before adding).  hconst / gconst override the constants (the bound's own test swaps two channels)."""
    x = P["x"].double()
    if hmode == "plain":
        h, hmag = x, x.abs()
    else:
        a, b = hconst or h_constants(P, hmode)
        h, hmag = a * x + b, a.abs() * x.abs() + b.abs()
        if hmode == "bn_relu":
            h = h.clamp_min(0.0)
    dy = P["dy"].double()
    if gmode == "plain":
        g, gmag = dy, dy.abs()
    else:
        a, b, cm, cs = (gconst or g_constants(P))[:4]
        y = P["y"].double()
        g = a * dy + b * y + cm + cs
        gmag = a.abs() * dy.abs() + b.abs() * y.abs() + cm.abs() + cs.abs()
    return h, g, hmag, gmag


def bound(P, geom, dt, hmag, gmag):
    """E = (2 u_T + (K + 16) 2^-24) W(gmag, hmag), elementwise, from the reference side only.  2 u_T: each operand is rounded to
    T once (relative u_T each; fp32: none).  K 2^-24: the fp32 accumulation over K = B Ho Wo pixels.  16: the fp32 roundings of
    the per-channel constants (src_raw_finish) and the two fused multiply-adds of the transform."""
    B, Hi, Wi, ks, s = GEOMS[geom]
    Ho, Wo = out_hw(geom)
    K = B * Ho * Wo
    return (2 * U_T[TYPES[dt][0]] + (K + 16) * 2.0 ** -24) * wgrad_fp64(hmag, gmag, ks, s)


@functools.lru_cache(maxsize=None)
def xform_reference(geom, Ci, Co, dt, hmode, gmode):
    P = xform_problem(geom, Ci, Co, dt)
    h, g, hmag, gmag = transformed(P, hmode, gmode)
    ks, s = GEOMS[geom][3:]
    return wgrad_fp64(h, g, ks, s), bound(P, geom, dt, hmag, gmag)


# ------------------------------------------------------------------------------------------------ stride-2 data gradient
DGRAD_SHAPES = [(3, 13, 11), (2, 24, 18)]   # (B, H, W) of the stride-2 conv's INPUT: -> 7x6 ((Ho + 1) / 2 odd case) and 12x9
DGRAD_CHANNELS = [(32, 32), (32, 64), (64, 32), (128, 128)]


@functools.lru_cache(maxsize=None)
def dgrad_problem(B, H, W, Ci, Co):
    """Integer gradient g [B, Ho, Wo, Co], integer forward weights w [Co][3][3][Ci], the fp64 data gradient [B, H, W, Ci], an
    integer addend, and the BatchNorm whose ReLU gates dx: x0 [B, H, W, Ci] with gamma, beta (deviations of at least 0.5, so
    that the mask argument a x0 + b is rarely within 1e-3 of zero)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = int_tensor((B, Ho, Wo, Co), 3000 + Ci + 3 * Co)
    w = int_tensor((Co, 3, 3, Ci), 4000 + Ci + 3 * Co)
    gen = torch.Generator().manual_seed(5000 + Ci + 3 * Co)
    x0 = torch.randn(B, H, W, Ci, generator=gen, dtype=torch.float64) * spread(Ci, 0.5, 2.0, gen) + spread(Ci, 0.25, 1.0, gen)
    return {"g": g, "w": w, "dx": dgrad_fp64(g, w, H, W), "addend": int_tensor((B, H, W, Ci), 6000 + Ci + 3 * Co), "x0": x0,
            "gamma": spread(Ci, 0.5, 2.0, gen).float(), "beta": (spread(Ci, 0.25, 1.0, gen) - 0.6).float()}


def dgrad_mask_argument(x0_stored, gamma, beta):
    """fp64 a x0 + b of the BatchNorm (batch statistics of the STORED x0) whose ReLU gates the data gradient."""
    f = x0_stored.double().reshape(-1, x0_stored.shape[-1])
    a = gamma.double() / torch.sqrt(f.var(0, unbiased=False) + EPS)
    return a * x0_stored.double() + (beta.double() - f.mean(0) * a)
