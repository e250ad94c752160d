"""Person-box handling on the GPU (mirror of reference ``src/lib/bounding_box.py``).

``bbox_filtering`` and ``bbox_nms`` run as ONE ``stlpose::box_select`` launch for all images of a batch (csrc/topdown.hip): the
reference walks every box in Python and calls torchvision.ops.nms per image.  ``get_detections`` / ``reshape_detection`` are cold
code on torch ops; ``bbox_to_image_keypoints`` is vectorised numpy.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)


def _device(xs) -> torch.device:
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda")


def _cat(parts, dtype, width, dev) -> torch.Tensor:
    ts = [torch.as_tensor(np.asarray(p) if not torch.is_tensor(p) else p).to(dev, dtype).reshape(-1, *width) for p in parts]
    return torch.cat(ts) if ts else torch.zeros(0, *width, dtype=dtype, device=dev)


def select_boxes(boxes: Sequence, scores: Sequence, labels=None, label: int = 1, score_thr=None, iou_thr: float = -1.0):
    """One box_select over per-image lists: boxes[i] [n_i, 4] (x1, y1, x2, y2), scores[i] [n_i], labels[i] [n_i] or None.
    Returns the kept image-local row indices per image (int64 numpy arrays; score order under NMS, input order otherwise)."""
    dev = _device(list(boxes) + list(scores))
    counts = [len(s) for s in scores]
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    b = _cat(boxes, torch.float32, (4,), dev)
    s = _cat(scores, torch.float32, (), dev).reshape(-1)
    lab = _cat(labels, torch.int64, (), dev).reshape(-1) if labels is not None else None
    keep, count = torch.ops.stlpose.box_select(b, s, lab, off, int(label), score_thr, float(iou_thr))
    keep, count = keep.cpu().numpy(), count.cpu().numpy()
    return [keep[o:o + c].astype(np.int64) for o, c in zip(off[:-1].tolist(), count.tolist())]


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def bbox_filtering(predictions, filter_=1, thr=0.6):
    """lib/bounding_box.py:127-168: keep the boxes with label == filter_ and score > thr (float32 comparison, as the reference's
    0-d tensors compare), in detector order.  predictions: the detector's list of {"boxes", "labels", "scores"} per image (torch
    tensors on any device, or arrays).  Returns per-image (boxes float32 [k, 4], labels int64 [k], scores float32 [k]) lists; the
    reference returns lists of per-box scalars, which np.asarray turns into the same arrays."""
    boxes = [p["boxes"] for p in predictions]
    labels = [p["labels"] for p in predictions]
    scores = [p["scores"] for p in predictions]
    kept = select_boxes(boxes, scores, labels, label=int(filter_), score_thr=float(np.float32(thr)), iou_thr=-1.0)
    fb, fl, fs = [], [], []
    for b, l, s, k in zip(boxes, labels, scores, kept):
        fb.append(_host(b).astype(np.float32).reshape(-1, 4)[k])
        fl.append(_host(l).astype(np.int64).reshape(-1)[k])
        fs.append(_host(s).astype(np.float32).reshape(-1)[k])
    return fb, fl, fs


def bbox_nms(boxes, labels, scores, nms_thr=0.5):
    """lib/bounding_box.py:171-206 with torchvision.ops.nms semantics (stable descending score order; a box is dropped when its
    IoU with a kept box exceeds nms_thr).  Per-image lists in, per-image lists of (boxes [k, 4], labels [k], scores [k]) out, in
    score order.  Differences from the reference: an image without boxes gives empty arrays (the reference raises on it), and
    the result is a list per image (the reference's np.array of the list fails when images keep different numbers of boxes)."""
    bs = [_host(b).astype(np.float32).reshape(-1, 4) for b in boxes]
    ss = [_host(s).astype(np.float32).reshape(-1) for s in scores]
    ls = [_host(l).reshape(-1) for l in labels]
    kept = select_boxes(bs, ss, None, score_thr=None, iou_thr=float(nms_thr))
    return [b[k] for b, k in zip(bs, kept)], [l[k] for l, k in zip(ls, kept)], [s[k] for s, k in zip(ss, kept)]


def reshape_detection(img, bb, height=256, width=192, offset=0):
    """lib/bounding_box.py:46-77: crop img [3, H, W] to the box (y0, x0, y1, x1), rounded to integers and grown by offset,
    and resize it to (height, width) with bilinear align_corners=True.  Returns [1, 3, height, width]."""
    y0, x0, y1, x1 = (int(round(float(v))) for v in bb)
    y0, x0, y1, x1 = y0 - offset, x0 - offset, y1 + offset, x1 + offset
    crop = img[:, y0:y1, x0:x1].reshape(1, 3, y1 - y0, x1 - x0)
    return F.interpolate(crop.clone().detach(), (height, width), mode="bilinear", align_corners=True)


def get_detections(imgs, bboxes, height=256, width=192):
    """lib/bounding_box.py:13-43: every box of every image as one [n, 3, height, width] batch ([] when there is none)."""
    dets = [reshape_detection(imgs[i], b, height=height, width=width)[0] for i, img_bbs in enumerate(bboxes) for b in img_bbs]
    return torch.stack(dets) if dets else []


def bbox_to_image_keypoints(pred_keypoints, list_bboxes, height=256, width=192, offset=0):
    """lib/bounding_box.py:80-124 vectorised: keypoints [n, J, 2] in (row, col) crop coordinates of the boxes (y0, x0, y1, x1)
    -> rounded integer image coordinates; keypoints that were -1 stay -1.  Like the reference it rescales pred_keypoints in
    place, and returns it unchanged when there are no boxes."""
    if sum(len(b) for b in list_bboxes) == 0:
        return pred_keypoints
    bx = np.concatenate([np.array(b) for b in list_bboxes if len(b) > 0]).reshape(-1, 4)
    n = len(bx)
    missing = pred_keypoints[:n] == -1
    y0, x0 = bx[:, 0] - offset, bx[:, 1] - offset
    hr = (bx[:, 2] - bx[:, 0] + 2 * offset) / height
    wr = (bx[:, 3] - bx[:, 1] + 2 * offset) / width
    pred_keypoints[:n, :, 0] = pred_keypoints[:n, :, 0] * hr[:, None] + y0[:, None]
    pred_keypoints[:n, :, 1] = pred_keypoints[:n, :, 1] * wr[:, None] + x0[:, None]
    out = np.round(np.array(pred_keypoints[:n])).astype(int)
    out[missing] = -1
    return out
