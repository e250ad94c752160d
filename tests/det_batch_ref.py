"""The numpy yardstick of stlpose::det_batch (csrc/det_batch.hip): stage 1 (ResizeImageDetection with the library's statement of
cv2.resize INTER_LINEAR, blended in float32 and rounded to the nearest-even level), the scaled boxes and the horizontal flip, written
from include/stlpose_hip_det_batch.h and independent of stlpose_amd.det_data.  The canvas has no yardstick here: the tests hold it to
stl_det_preprocess, the kernel it replaces, bit for bit."""
import numpy as np

f32 = np.float32


def resized_size(h: int, w: int, s1: int):
    """(scale, rh, rw) of custom_transforms.py:49-57."""
    if h > w:
        scale = s1 / h
        return scale, s1, int(w * scale)
    scale = s1 / w
    return scale, int(h * scale), s1


def taps(n_out: int, n_in: int):
    """lin_tap of csrc/detector.hip for every output index: (i0, i1, w0, w1)."""
    scale = 1.0 / (n_out / n_in)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
    i = np.floor(f).astype(np.int64)
    a = (f - i.astype(f32)).astype(f32)
    lo = i < 0
    i[lo], a[lo] = 0, 0
    hi = i >= n_in - 1
    i[hi], a[hi] = n_in - 1, 0
    return i, np.minimum(i + 1, n_in - 1), (f32(1) - a).astype(f32), a


def stage1(img: np.ndarray, s1: int, flip: bool = False) -> np.ndarray:
    """uint8 HWC -> uint8 [s1, s1, 3]: the rh x rw resize at the top left, zeros elsewhere; flip mirrors the region's columns."""
    h, w = img.shape[:2]
    _, rh, rw = resized_size(h, w, s1)
    y0, y1, wy0, wy1 = taps(rh, h)
    x0, x1, wx0, wx1 = taps(rw, w)
    x = img.astype(f32)
    top = (x[y0][:, x0] * wx0[None, :, None]).astype(f32) + (x[y0][:, x1] * wx1[None, :, None]).astype(f32)
    bot = (x[y1][:, x0] * wx0[None, :, None]).astype(f32) + (x[y1][:, x1] * wx1[None, :, None]).astype(f32)
    val = (top * wy0[:, None, None]).astype(f32) + (bot * wy1[:, None, None]).astype(f32)
    region = np.rint(val).astype(np.uint8)   # nearest even
    if flip:
        region = region[:, ::-1]
    out = np.zeros((s1, s1, 3), np.uint8)
    out[:rh, :rw] = region
    return out


def scaled_boxes(boxes: np.ndarray, h: int, w: int, s1: int, flip: bool = False) -> np.ndarray:
    """float32 [n, 4] xyxy in source pixels -> on the s1 x s1 image: times float32(scale) in float32; flipped (rw - 1 - x2, y1,
    rw - 1 - x1, y2) in float32."""
    scale, _, rw = resized_size(h, w, s1)
    b = (np.asarray(boxes, f32).reshape(-1, 4) * f32(scale)).astype(f32)
    if flip:
        edge = f32(rw - 1)
        b = np.stack([edge - b[:, 2], b[:, 1], edge - b[:, 0], b[:, 3]], 1).astype(f32)
    return b


def gt_table(boxes_per_image, labels_per_image, sizes, s1: int, ratio_x: float, ratio_y: float, flips=None):
    """(gt float32 [rows, 5], offsets int32 [B + 1]): the scaled boxes times the float64 canvas ratios in float64, rounded once."""
    rows, offsets = [], [0]
    for i, (b, l, (h, w)) in enumerate(zip(boxes_per_image, labels_per_image, sizes)):
        sb = scaled_boxes(b, h, w, s1, bool(flips[i]) if flips is not None else False).astype(np.float64)
        g = np.concatenate([sb * np.array([ratio_x, ratio_y, ratio_x, ratio_y]), (np.asarray(l, np.int64) - 1)[:, None].astype(np.float64)], 1)
        rows.append(g.astype(f32))
        offsets.append(offsets[-1] + len(l))
    return np.concatenate(rows, 0).reshape(-1, 5), np.asarray(offsets, np.int32)
