"""Numpy yardstick of the fused evaluation tail (stlpose::eval_tail / eval_affine, stlpose_amd/csrc/eval_tail.hip), and the data
its tests share.

Every element step is done in np.float32 exactly as the kernels state it -- merged = 0.5 * (a + shift(flip_back(bflip))), d =
(merged - target) * w -- the squared error is summed in float64, arg-max is np.argmax (first maximum, NaN first), the refinement
and the inverse crop transform are those of oracle/pose_ref.py (refine_quarter_pixel, affine_from_box with inv=True) with the
kernels' number formats: coordinates float32, centre and scale rounded to float32, the transform in float64, the result cast to
float32.  tests/test_eval_tail_cpu.py pins this file against the oracle's own functions."""
import numpy as np

FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
SHAPES = [(3, 17, 5, 7), (2, 3, 8, 6), (1, 17, 64, 48), (2, 17, 96, 72), (5, 17, 33, 31)]
F = np.float32


def perm(j):
    p = list(range(j))
    for a, b in FLIP_PAIRS:
        if a < j and b < j:
            p[a], p[b] = b, a
    return np.asarray(p, np.int32)


def merge(a, bflip):
    """forward_pass(flip=True) after the two forwards: flip_back, 1-px right shift with column 0 kept, average; fp32."""
    a = np.asarray(a, F)
    if bflip is None:
        return a
    f = np.asarray(bflip, F)[:, perm(a.shape[1])][:, :, :, ::-1]
    shifted = f.copy()
    shifted[:, :, :, 1:] = f[:, :, :, :-1]
    return F(0.5) * (a + shifted)


def max_preds(hm):
    """(masked coordinates float32 [B, J, 2], maxval float32 [B, J]) as stl_heatmap_argmax writes them."""
    b, j, h, w = hm.shape
    flat = hm.reshape(b, j, -1)
    idx = np.argmax(flat, 2)
    mx = np.take_along_axis(flat, idx[..., None], 2)[..., 0]
    xy = np.stack([(idx % w).astype(F), (idx // w).astype(F)], -1)
    return xy * (mx > 0)[..., None].astype(F), mx


def refine(hm, xy):
    """+-0.25 px towards the higher neighbour, strict interior (oracle.pose_ref.refine_quarter_pixel); a zero or unordered
    difference moves nothing."""
    out = xy.copy()
    _, _, h, w = hm.shape
    for n in range(xy.shape[0]):
        for p in range(xy.shape[1]):
            px, py = int(np.floor(xy[n, p, 0] + F(0.5))), int(np.floor(xy[n, p, 1] + F(0.5)))
            if 1 < px < w - 1 and 1 < py < h - 1:
                dx = hm[n, p, py, px + 1] - hm[n, p, py, px - 1]
                dy = hm[n, p, py + 1, px] - hm[n, p, py - 1, px]
                out[n, p, 0] += F(0.25) if dx > 0 else (F(-0.25) if dx < 0 else F(0))
                out[n, p, 1] += F(0.25) if dy > 0 else (F(-0.25) if dy < 0 else F(0))
    return out


def tail(a, bflip, target, tweight):
    """One batch -> dict(merged, pred_xy, tgt_xy, coords, maxval, partial float64 [B, J], loss float64)."""
    m = merge(a, bflip)
    t = np.asarray(target, F)
    b, j, h, w = m.shape
    pred_xy, maxval = max_preds(m)
    tgt_xy, _ = max_preds(t)
    with np.errstate(invalid="ignore"):
        d = (m - t) * np.asarray(tweight, F).reshape(b, j, 1, 1)
    partial = (d.astype(np.float64) ** 2).reshape(b, j, -1).sum(2)
    return dict(merged=m, pred_xy=pred_xy, tgt_xy=tgt_xy, coords=refine(m, pred_xy), maxval=maxval, partial=partial,
                loss=partial.sum() * 0.5 / (b * j * h * w))


def affine(coords, maxval, center, scale, h, w):
    """preds float32 [N, J, 3]: the inverse crop transform (rot = 0, s = W / (scale_x * 200) on both axes) and maxval."""
    c, sc = np.asarray(center, F).astype(np.float64), np.asarray(scale, F).astype(np.float64)
    s = (w / (sc[:, 0] * 200.0))[:, None]
    x = (coords[..., 0].astype(np.float64) - 0.5 * w) / s + c[:, 0:1]
    y = (coords[..., 1].astype(np.float64) - 0.5 * h) / s + c[:, 1:2]
    return np.stack([x.astype(F), y.astype(F), np.asarray(maxval, F)], -1)


def float32_neighbours(v):
    """np.float32 of the float64 v and the float32 on either side of it."""
    f = F(v)
    return {float(np.nextafter(f, F(-np.inf))), float(f), float(np.nextafter(f, F(np.inf)))}


# ------------------------------------------------------------------------------------------------ shared data
def case(shape, seed=0, nan=False):
    """Random maps with the planted cases of the issue on as many (person, joint) slots as the shape has, in this order: a
    duplicated maximum; a tie that only the flip average creates; an all-negative and an all-zero map; a maximum on each border
    and in column / row 1 and W-2 / H-2; an isolated interior maximum (dx == dy == 0); target maps that are all zero and that
    have a duplicated maximum.  Person 0 (when B > 1) has zero target weights.  nan=True: one NaN in the last slot of a.
    A planted slot has a zero mirrored source, so its merged map is exactly 0.5 * a.  -> (a, bflip, target, tweight)."""
    b, j, h, w = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    a = (rng.random(shape) * 1.2 - 0.2).astype(F)
    bf = (rng.random(shape) * 1.2 - 0.2).astype(F)
    t = rng.random(shape).astype(F)
    tw = rng.choice(np.asarray([0.0, 0.5, 1.0, 1.0], F), (b, j, 1))
    if b > 1:
        tw[0] = 0
    p = perm(j)
    slots = [(n, c) for c in range(j) for n in range(b)]
    yi, xi = h // 2, w // 2   # interior whenever the map has an interior

    def peak(n, c, y, x):
        a[n, c, y, x] = 8.0   # merged >= 3.9, everything else stays below 1

    def dup(n, c):
        a[n, c], bf[n, p[c]] = 0, 0
        a[n, c, 1, 2] = a[n, c, h - 2, 1] = 2.0

    def flip_tie(n, c):       # a alone peaks at (yi, xi); the average lifts the earlier pixel (1, 1) to the same 0.5
        a[n, c], bf[n, p[c]] = 0, 0
        a[n, c, yi, xi], a[n, c, 1, 1] = 1.0, 0.5
        bf[n, p[c], 1, w - 1] = 0.5   # read by x = 1 (and by x = 0, where a is 0: merged 0.25)

    def negative(n, c):
        a[n, c] = -0.1 - rng.random((h, w)).astype(F)
        bf[n, p[c]] = -0.1 - rng.random((h, w)).astype(F)

    def zero(n, c):
        a[n, c], bf[n, p[c]] = 0, 0

    def isolated(n, c):
        a[n, c], bf[n, p[c]] = 0, 0
        a[n, c, yi, xi] = 1.0

    def target_zero(n, c):
        t[n, c] = 0

    def target_dup(n, c):
        t[n, c, 2, 3] = t[n, c, h - 1, 0] = 5.0

    plants = [dup, flip_tie, negative, zero] \
        + [lambda n, c, y=y, x=x: peak(n, c, y, x) for y, x in ((0, xi), (h - 1, xi), (yi, 0), (yi, w - 1), (1, xi), (h - 2, xi), (yi, 1), (yi, w - 2))] \
        + [isolated, target_zero, target_dup]
    for (n, c), plant in zip(slots, plants):
        plant(n, c)
    if nan:
        n, c = slots[-1]
        a[n, c, h // 3, w // 3] = np.nan
    return a, bf, t, tw
