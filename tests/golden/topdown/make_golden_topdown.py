#!/usr/bin/env python3
"""Generate g14_topdown.npz by running the REFERENCE's own lib/bounding_box.py, lib/pose_parsing.py and lib/transforms.py
(TransformDetection._coords2cs, get_affine_transform).

Runs only where the reference tree exists.  Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/topdown/make_golden_topdown.py
(STL_GOLDEN_OUT=<dir> writes elsewhere).  torchvision and cv2 are stub modules: cv2.getAffineTransform is the exact 3-point solve
of tests/golden/make_golden.py, and torchvision.ops.nms is tests/topdown_ref.nms -- so the NMS semantics are pinned by that
restatement only; what the fixture pins from the reference is everything around it (filtering, per-image lists, order of the
gathered boxes, labels and scores).  Only inputs and outputs are stored.

Contents:
  det_boxes [N,4] f32 / det_labels [N] i64 / det_scores [N] f32 / det_offsets [I+1]: a ragged detector output (images of 0, 1, 9,
    40 and 120 rows) with duplicate, contained and zero-area boxes and exact score ties;
  filt_{boxes,labels,scores,count}: bbox_filtering(filter_=1, thr=0.6), concatenated per image;
  nms_raw_<t>_{idx,count}: bbox_nms on every row of each non-empty image (t = 0.3, 0.5, 0.7), as image-local row indices;
  nms_filt_{boxes,labels,scores,count}: bbox_nms(nms_thr=0.5) on the filtered lists;
  hm [4,17,64,48]: heat maps (one all-negative map, one constant map); cpo_entries [4,19], cpo_all [68,4]: create_pose_from_outputs;
  ce_keypoints [3,17,2] (with -1 rows), ce_maxvals, ce_entries, ce_all: create_pose_entries;
  rdb_joints [4,17,3]: 05_create_archdata_retrieval_db.py's (x, y, vis) conversion of each person's map, one person per batch;
  td_coords [M,4] f32, td_centers, td_scales, td_trans [M,2,3]: TransformDetection(192, 256)._coords2cs and get_affine_transform;
  gd_imgs [2,3,40,30], gd_boxes [4,4] (y0,x0,y1,x1), gd_counts, gd_crops [4,3,32,24]: get_detections(height=32, width=24);
  bk_pred [3,17,2] (with -1), bk_boxes [3,4], bk_out: bbox_to_image_keypoints.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
OUT = os.environ.get("STL_GOLDEN_OUT") or HERE
REF = "/root/reference/src"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import topdown_ref  # noqa: E402

NMS_THRS = (0.3, 0.5, 0.7)


def _import_reference():
    for name in ("torchvision", "torchvision.ops", "torchvision.transforms", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].ops = sys.modules["torchvision.ops"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]

    def _nms(boxes, scores, iou_threshold):
        return torch.from_numpy(topdown_ref.nms(boxes.numpy(), scores.numpy(), iou_threshold))

    def _get_affine(src, dst):
        a = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], 1)
        return np.linalg.solve(a, np.asarray(dst, np.float64)).T
    sys.modules["torchvision.ops"].nms = _nms
    sys.modules["cv2"].getAffineTransform = _get_affine
    sys.path.insert(0, REF)
    import lib.bounding_box as bb
    import lib.pose_parsing as pp
    import lib.transforms as tf
    return bb, pp, tf


def detections(rng):
    sizes = (0, 1, 9, 40, 120)
    boxes, labels, scores = [], [], []
    for n in sizes:
        xy = rng.uniform(0, 400, (n, 2))
        wh = rng.uniform(5, 120, (n, 2))
        b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        s = rng.uniform(0, 1, n).astype(np.float32)
        lab = np.where(rng.uniform(size=n) < 0.8, 1, rng.integers(2, 5, n)).astype(np.int64)
        if n >= 9:
            b[1] = b[0]                                        # duplicate, same score: a tie
            s[1] = s[0] = max(s[0], np.float32(0.7))
            lab[0] = lab[1] = 1
            b[2] = b[0] + np.array([4, 4, -4, -4], np.float32)  # contained
            b[3, 2:] = b[3, :2]                                # zero area
            b[4, 2] = b[4, 0]                                  # zero width
            s[5] = s[6] = np.float32(0.8125)                  # exact tie, different boxes
            lab[5] = lab[6] = 1
            s[7] = np.float32(0.6)                             # exactly the filter threshold (not kept: score > thr)
            lab[7] = 1
        if n >= 40:
            b[20:30] = b[10] + rng.uniform(-6, 6, (10, 4)).astype(np.float32)   # a cluster around one person
            s[20:30] = np.float32(0.9)
            lab[20:30] = 1
        boxes.append(b), labels.append(lab), scores.append(s)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(boxes), np.concatenate(labels), np.concatenate(scores), off


def heatmaps(rng):
    n, j, h, w = 4, 17, 64, 48
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    hm = np.zeros((n, j, h, w), np.float32)
    for p in range(n):
        for k in range(j):
            cy, cx = rng.uniform(2, h - 3), rng.uniform(2, w - 3)
            s = rng.uniform(1.5, 3.0)
            hm[p, k] = rng.uniform(0.05, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            hm[p, k] += rng.normal(0, 0.02, (h, w)).astype(np.float32)
    hm[2, 5] = -rng.uniform(0.1, 1.0, (h, w)).astype(np.float32)   # all negative: preds 0
    hm[3, 7] = np.float32(0.25)                                    # constant: index 0
    return (np.round(hm * 8192) / 8192).astype(np.float32)         # 13 fractional bits: the file compresses


def check_gaps(hm):
    up = F.interpolate(torch.from_numpy(hm), (256, 192), mode="bilinear", align_corners=True).numpy().reshape(hm.shape[0], 17, -1)
    for p in range(hm.shape[0]):
        for k in range(17):
            v = up[p, k]
            if p == 3 and k == 7:
                assert np.all(v == v[0]), "the constant map must upsample to a constant"
                continue
            top = np.sort(v)[-2:]
            assert top[1] - top[0] > 1e-4 * abs(top[1]), (p, k, top)


def main():
    bb, pp, tf = _import_reference()
    rng = np.random.default_rng(20261016)
    out = {}
    boxes, labels, scores, off = detections(rng)
    out.update(det_boxes=boxes, det_labels=labels, det_scores=scores, det_offsets=off)
    preds = [{"boxes": torch.from_numpy(boxes[a:b]), "labels": torch.from_numpy(labels[a:b]), "scores": torch.from_numpy(scores[a:b])}
             for a, b in zip(off[:-1], off[1:])]
    fb, fl, fs = bb.bbox_filtering(preds, filter_=1, thr=0.6)
    out["filt_boxes"] = np.array([x for img in fb for x in img], np.float32).reshape(-1, 4)
    out["filt_labels"] = np.array([x for img in fl for x in img], np.int64)
    out["filt_scores"] = np.array([x for img in fs for x in img], np.float32)
    out["filt_count"] = np.array([len(x) for x in fb], np.int64)
    for t in NMS_THRS:
        idx, cnt = [], []
        for a, b in zip(off[:-1], off[1:]):
            if b == a:                                  # the reference cannot take an image without boxes
                cnt.append(0)
                continue
            kb, kl, ks = bb.bbox_nms([list(boxes[a:b])], [list(np.arange(b - a))], [list(scores[a:b])], nms_thr=t)
            idx.append(np.asarray(kl[0], np.int64)), cnt.append(len(kl[0]))
            assert np.array_equal(kb[0], boxes[a:b][kl[0]])
        out[f"nms_raw_{t}_idx"], out[f"nms_raw_{t}_count"] = np.concatenate(idx), np.array(cnt, np.int64)
    nb, nl, ns, nc = [], [], [], []
    for b_, l_, s_ in zip(fb, fl, fs):
        if len(b_) == 0:
            nc.append(0)
            continue
        kb, kl, ks = bb.bbox_nms([b_], [l_], [s_], nms_thr=0.5)
        nb.append(kb[0].astype(np.float32)), nl.append(kl[0].astype(np.int64)), ns.append(ks[0].astype(np.float32)), nc.append(len(kb[0]))
    out.update(nms_filt_boxes=np.concatenate(nb), nms_filt_labels=np.concatenate(nl), nms_filt_scores=np.concatenate(ns),
               nms_filt_count=np.array(nc, np.int64))

    hm = heatmaps(rng)
    check_gaps(hm)
    out["hm"] = hm
    ent, allk = pp.create_pose_from_outputs(torch.from_numpy(hm), keypoint_thr=0.1)
    out["cpo_entries"], out["cpo_all"] = np.stack(ent), np.asarray(allk)
    joints = []
    for p in range(hm.shape[0]):   # 05_create_archdata_retrieval_db.py:128-150, one person per loader batch
        scaled = F.interpolate(torch.from_numpy(hm[p:p + 1]), (256, 192), mode="bilinear", align_corners=True)
        kc, mv = pp.get_max_preds_hrnet(scaled.cpu().numpy())
        _, ak = pp.create_pose_entries(keypoints=kc, max_vals=mv, thr=0.1)
        ak = np.array([ak[:, 1], ak[:, 0], ak[:, 2], ak[:, 3]]).T
        joints.append(torch.Tensor(np.array((ak[:, 1], ak[:, 0], ak[:, -1])).T).float().numpy())
    out["rdb_joints"] = np.stack(joints)

    kp = rng.uniform(0, 190, (3, 17, 2)).astype(np.float32)
    kp[0, 3] = -1
    kp[1, 4, 1] = -1
    kp[2, 10, 0] = -1
    mv = rng.uniform(0, 0.3, (3, 17, 1)).astype(np.float32)
    ent, allk = pp.create_pose_entries(kp, mv, thr=0.1)
    out.update(ce_keypoints=kp, ce_maxvals=mv, ce_entries=np.stack(ent), ce_all=np.asarray(allk))

    det = tf.TransformDetection(det_width=192, det_height=256)
    coords = np.concatenate([boxes[off[4] + 30:off[4] + 42], np.array([[10, 10, 200, 30], [10, 10, 30, 300], [0, 0, 96, 128],
                                                                 [-2.0, 5, 0.0, 9]], np.float32)]).astype(np.float32)
    cs = [det._coords2cs(list(c)) for c in coords]
    out["td_coords"] = coords
    out["td_centers"] = np.stack([c for c, _ in cs])
    out["td_scales"] = np.stack([s for _, s in cs])
    out["td_trans"] = np.stack([tf.get_affine_transform(center=c, scale=s, rot=0, output_size=det.image_size) for c, s in cs])

    imgs = torch.from_numpy(rng.uniform(0, 255, (2, 3, 40, 30)).astype(np.float32))
    gb = [[np.array([3.4, 2.5, 30.6, 20.0]), np.array([0, 0, 40, 30])], [np.array([10.0, 5.0, 21.5, 17.49]), np.array([1, 1, 2, 2])]]
    crops = bb.get_detections(imgs, gb, height=32, width=24)
    out.update(gd_imgs=imgs.numpy(), gd_boxes=np.array([b for img in gb for b in img], np.float64), gd_counts=np.array([2, 2]),
               gd_crops=crops.numpy())

    pk = rng.uniform(0, 50, (3, 17, 2)).astype(np.float32)
    pk[0, 2] = -1
    pk[2, 5, 1] = -1
    bxs = [np.array([[5.0, 7.0, 105.0, 70.0]], np.float32), np.zeros((0, 4), np.float32),
           np.array([[0.0, 0.0, 64.0, 48.0], [13.5, 2.25, 77.0, 99.0]], np.float32)]
    out["bk_pred"], out["bk_boxes"] = pk.copy(), np.concatenate(bxs)
    out["bk_out"] = bb.bbox_to_image_keypoints(pk.copy(), [list(b) for b in bxs], height=256, width=192)
    np.savez_compressed(os.path.join(OUT, "g14_topdown.npz"), **out)


if __name__ == "__main__":
    main()
