"""Host (numpy, float32) restatements of the top-down kernels' semantics, in the kernels' operation order:
torchvision.ops.nms as lib/bounding_box.py:171-206 calls it, and F.interpolate(bilinear, align_corners=True).
These are what the GPU results are held to, and what the fixture generator substitutes for torchvision.ops.nms."""
from __future__ import annotations

import numpy as np


def nms(boxes, scores, iou_thr):
    """torchvision.ops.nms: order by descending score (stable, NaN first), greedy suppression of every later box whose
    IoU with a kept box exceeds iou_thr.  area = (x2-x1)*(y2-y1), inter = max(0, min(x2)-max(x1)) * max(0, min(y2)-max(y1)),
    iou = inter / (area_kept + area_j - inter), all in float32; the float IoU is compared with the threshold in float64.
    Returns int64 indices in score order."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    s = np.asarray(scores, np.float32).reshape(-1)
    n = len(s)
    if n == 0:
        return np.zeros(0, np.int64)
    key = np.where(np.isnan(s), np.float32(np.inf), s)
    order = np.lexsort((np.arange(n), -np.isnan(s).astype(np.int8), -key.astype(np.float64)))
    x1, y1, x2, y2 = b[order, 0], b[order, 1], b[order, 2], b[order, 3]
    area = (x2 - x1) * (y2 - y1)
    dead = np.zeros(n, bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            if dead[i]:
                continue
            keep.append(order[i])
            j = np.arange(i + 1, n)
            xx1 = np.where(x1[i] < x1[j], x1[j], x1[i])
            yy1 = np.where(y1[i] < y1[j], y1[j], y1[i])
            xx2 = np.where(x2[j] < x2[i], x2[j], x2[i])
            yy2 = np.where(y2[j] < y2[i], y2[j], y2[i])
            dw, dh = xx2 - xx1, yy2 - yy1
            w = np.where(np.float32(0) < dw, dw, np.float32(0))
            h = np.where(np.float32(0) < dh, dh, np.float32(0))
            inter = w * h
            iou = inter / ((area[i] + area[j]) - inter)
            dead[j[iou.astype(np.float64) > float(iou_thr)]] = True
    return np.asarray(keep, np.int64)


def _taps(n_in, n_out):
    """Source index pair and weights per output coordinate (torch's align_corners=True rule, float32)."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = np.float32(scale) * np.arange(n_out, dtype=np.float32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def resize_bilinear(hm, ho, wo):
    """F.interpolate(hm, (ho, wo), mode="bilinear", align_corners=True) on [..., H, W], float32: W first within each row, then
    the rows, nothing fused; the identity size is a copy."""
    x = np.asarray(hm, np.float32)
    h, w = x.shape[-2:]
    if (h, w) == (ho, wo):   # torch copies at the identity size
        return x.copy()
    ry0, ry1, ly0, ly1 = _taps(h, ho)
    cx0, cx1, lx0, lx1 = _taps(w, wo)
    with np.errstate(invalid="ignore", over="ignore"):
        top = lx0 * x[..., ry0, :][..., cx0] + lx1 * x[..., ry0, :][..., cx1]
        bot = lx0 * x[..., ry1, :][..., cx0] + lx1 * x[..., ry1, :][..., cx1]
        return ly0[:, None] * top + ly1[:, None] * bot


def argmax_first(flat):
    """np.argmax order of stl_heatmap_argmax over the last axis: the first NaN, else the first maximum."""
    f = np.asarray(flat)
    nan = np.isnan(f)
    return np.where(nan.any(-1), nan.argmax(-1), np.nanargmax(np.where(nan, -np.inf, f), -1) if f.size else 0)
