"""Heatmap decode on device (mirror of reference ``src/lib/pose_parsing.py`` / ``lib/metrics.py``)."""
from __future__ import annotations

import numpy as np
import torch

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)


def _dev(x, device=None) -> torch.Tensor:
    if torch.is_tensor(x):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(x))
    if not t.is_cuda:
        t = t.to(device or "cuda")
    return t.contiguous().float()


def max_preds_device(hm: torch.Tensor):
    """-> (idx int32 (B,J), maxvals f32 (B,J,1), preds f32 (B,J,2)) as device tensors."""
    return torch.ops.stlpose.heatmap_argmax(hm)   # custom op -> stl_heatmap_argmax (ops.py)


def get_max_preds_hrnet(scaled_heats, thr=0.1):
    """reference lib/pose_parsing.py:16-55 (numpy in, numpy out; empty batch -> ([], []))."""
    if scaled_heats.shape[0] == 0:
        return [], []
    hm = _dev(scaled_heats)
    _, mx, preds = max_preds_device(hm)
    return preds.cpu().numpy(), mx.cpu().numpy()


def get_final_preds_hrnet(heatmaps, center, scale):
    """reference lib/pose_parsing.py:58-92: argmax, +-0.25 px refinement, inverse crop affine
    (rot = 0).  Returns (preds, maxvals, coords) like the reference."""
    hm = _dev(heatmaps)
    b, j, h, w = hm.shape
    c = _dev(np.asarray(center, dtype=np.float32), hm.device)
    s = _dev(np.asarray(scale, dtype=np.float32), hm.device)
    preds, mx = torch.ops.stlpose.final_preds(hm, c, s)   # custom op -> stl_final_preds
    p = preds.cpu().numpy()
    # coords in heatmap space = forward crop transform of preds (kept for API parity)
    sc = (w / (np.asarray(scale, dtype=np.float64)[:, 0] * 200.0))[:, None]
    ctr = np.asarray(center, dtype=np.float64)
    coords = np.stack([(p[..., 0] - ctr[:, None, 0]) * sc + 0.5 * w, (p[..., 1] - ctr[:, None, 1]) * sc + 0.5 * h], -1)
    return p, mx.cpu().numpy(), coords.astype(np.float32)


def pck_from_coords(pred, tgt, h, w, thr=0.5):
    """The host arithmetic of ``accuracy`` behind its two arg-max calls: pred, tgt [B, J, 2] (x, y; the masked integer coordinates
    of ``heatmap_argmax``) of maps of h x w -> (acc [J + 1], avg, cnt).  Keeps the reference's normalisation (x by h / 10, y by
    w / 10); a joint whose target has no coordinate above 1 in any sample counts as -1 and stays out of the average."""
    pred, tgt = np.asarray(pred), np.asarray(tgt)
    b, j = pred.shape[:2]
    norm = np.ones((b, 2)) * np.array([h, w]) / 10
    ok = (tgt[..., 0] > 1) & (tgt[..., 1] > 1)
    d = np.linalg.norm(pred / norm[:, None] - tgt / norm[:, None], axis=-1)
    acc = np.zeros(j + 1)
    tot, cnt = 0.0, 0
    for c in range(j):
        n = ok[:, c].sum()
        a = (d[:, c][ok[:, c]] < thr).sum() / n if n > 0 else -1
        acc[c + 1] = a
        if a >= 0:
            tot, cnt = tot + a, cnt + 1
    avg = tot / cnt if cnt else 0
    if cnt:
        acc[0] = avg
    return acc, avg, cnt


def accuracy(output, target, hm_type="gaussian", thr=0.5):
    """reference lib/metrics.py:321-364 (PCK on heatmap argmaxes; the corrupted line :355-356 read
    as ``acc[i + 1] = dist_acc(dists[idx[i]])``).  Argmax runs on device; the 2*B*17 distances are
    host arithmetic (``pck_from_coords``)."""
    o, t = _dev(output), _dev(target)
    _, _, pred = max_preds_device(o)
    _, _, tgt = max_preds_device(t)
    pred, tgt = pred.cpu().numpy(), tgt.cpu().numpy()
    h, w = o.shape[2:]
    acc, avg, cnt = pck_from_coords(pred, tgt, h, w, thr)
    return acc, avg, cnt, pred


def create_pose_entries(keypoints, max_vals=None, thr=0.1):
    """reference lib/pose_parsing.py:107-133, vectorised.  keypoints [n, 17, 2] -> (pose_entries: n arrays of 19 = keypoint row
    ids 17 * person + joint where x != -1, then the count, then -1; all_keypoints [n * 17, 4] rows (x, y, 1, vis): a row holding
    a -1 becomes all -1, vis = 0 where max_vals < thr).  The dtype is the reference's: float64 for float input, int64 for int."""
    if len(keypoints) == 0:
        return [], []
    kp = np.asarray(keypoints)
    n, j = kp.shape[:2]
    flat = kp.reshape(n * j, -1)
    all_kp = np.ones((n * j, flat.shape[1] + 2), np.result_type(kp.dtype, np.int64))
    all_kp[:, :flat.shape[1]] = flat
    all_kp[(all_kp == -1).any(1)] = -1
    if max_vals is not None:
        low = np.argwhere(np.asarray(max_vals)[:, :, 0] < thr)
        all_kp[low[:, 0] * 17 + low[:, 1], -1] = 0
    valid = kp[:, :, 0] != -1
    entries = -np.ones((n, 19))
    entries[:, :j] = np.where(valid, 17 * np.arange(n)[:, None] + np.arange(j), -1)
    entries[:, -2] = (entries[:, :-2] != -1).sum(1)
    return list(entries), all_kp


def create_pose_from_outputs(dets, keypoint_thr=0.1):
    """reference lib/pose_parsing.py:136-153: heat maps [B, 17, h, w] -> (pose_entries, all_keypoints [B * 17, 4] as (y, x, 1,
    vis)) at 256 x 192.  The upsample and argmax are one fused kernel (stlpose::heatmap_resize_argmax): the 256 x 192 maps are
    never written, only 17 x 3 numbers per person reach the host.  An empty batch gives ([], an empty [0, 4] array); the
    reference raises on it."""
    hm = dets if torch.is_tensor(dets) and dets.is_cuda else _dev(dets)
    if hm.shape[0] == 0:
        return [], np.zeros((0, 4))
    _, mx, preds = torch.ops.stlpose.heatmap_resize_argmax(hm.contiguous().float(), 256, 192)
    entries, all_kp = create_pose_entries(preds.cpu().numpy(), mx.cpu().numpy()[..., None], thr=keypoint_thr)
    return entries, all_kp[:, [1, 0, 2, 3]]
