#!/usr/bin/env python3
"""Generate g15_effdet.npz by running the REFERENCE's own EfficientDetBackbone (src/models/EfficientDet.py with
models/efficientdet_utils/* and models/efficientnet/*) on the CPU.

Runs only where the reference tree exists.  Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/detector/make_golden_detector.py
(STL_GOLDEN_OUT=<dir> writes elsewhere).  ``models`` is a bare package over the reference's models/ directory (its __init__
imports unrelated networks); torchvision and cv2 are stub modules: transforms.Normalize is (x - mean) / std in float32,
cv2.resize is tests/detector_ref.resize_linear and torchvision.ops.boxes.{nms, batched_nms} are the numpy restatements of
tests/detector_ref -- so resampling and NMS are pinned by those restatements only; everything else (weights layout, network,
anchors, decode, thresholds, invert_affine, output format) is the reference's.  Weights: tests/detector_ref.synth_state_dict.

Contents (D0, num_classes 1, B = 2 images of 300 x 400 and 480 x 360, CHW in [0, 1], stored as uint8 / 255):
  the images are tests/detector_ref.images() (seeded); canvas_s [2, 3, 64, 64]: the canvas at every 8th pixel;
  p{3,4,5}_s, f{0..4}_s: backbone outputs and BiFPN outputs at strided samples (every 4th of C, H, W), *_stats (mean, std, absmax);
  cls [2, A, 1]: the full classification; cand{i}_idx, cand{i}_reg: the regression rows of every anchor scoring above lo_thr
    (all that the postprocess reads at either threshold), reg_stats; anchors_sum: float64 checksum;
  det{i}_{boxes,labels,scores}: forward's dicts (threshold 0.5, iou 0.5); no candidate score lies within 1e-5 of the threshold
    and no IoU within 1e-4 of the NMS threshold (check_margins);
  lo_thr, lo{i}_{rois,class_ids,scores}: the reference postprocess at threshold lo_thr (> 4096 candidates in image 0), on the
    canvas, before invert_affine;
  d0_layout, d3_layout: the state_dict layout, "key shape" lines as uint8 text; d3_{reg,cls}_stats, d3_f_stats: D3 at B = 1 on img0.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
OUT = os.environ.get("STL_GOLDEN_OUT") or HERE
REF = "/root/reference/src"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import detector_ref as R  # noqa: E402

LO_THR = 0.2


def _import_reference():
    for name in ("torchvision", "torchvision.ops", "torchvision.ops.boxes", "torchvision.transforms", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tv = sys.modules["torchvision"]
    tv.ops, tv.transforms = sys.modules["torchvision.ops"], sys.modules["torchvision.transforms"]
    tv.ops.boxes = sys.modules["torchvision.ops.boxes"]

    def _nms(boxes, scores, thr):
        return torch.from_numpy(R.nms(boxes.numpy(), scores.numpy(), thr))

    def _bnms(boxes, scores, idxs, iou_threshold):
        return torch.from_numpy(R.batched_nms(boxes.numpy(), scores.numpy(), idxs.numpy(), iou_threshold))

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)

        def __call__(self, t):
            return (t - self.mean[:, None, None]) / self.std[:, None, None]
    tv.ops.boxes.nms, tv.ops.boxes.batched_nms = _nms, _bnms
    tv.transforms.Normalize = Normalize
    sys.modules["cv2"].resize = lambda img, dsize, interpolation=None: R.resize_linear(img, dsize[0], dsize[1])
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self   # the reference's preprocess moves the canvas to the GPU
    from models.EfficientDet import EfficientDetBackbone
    from models.efficientdet_utils import utils as U
    return EfficientDetBackbone, U


def stats(t):
    t = t.double()
    return np.array([t.mean().item(), t.std().item(), t.abs().max().item()])


def strided(t):
    return t[:, ::4, ::4, ::4].numpy().astype(np.float32)


def check_margins(boxes, scores, classes, thr, iou_thr, eps_score=1e-5, eps_iou=1e-4):
    """The candidates of one image (score > thr): no score within eps_score of thr and no pair of one class with an IoU within
    eps_iou of iou_thr.  Returns how many candidates have a near-tied overlapping rival (detector_ref.near_ties): the
    reference's own scores hold such rows, so a network that agrees with it to ~1e-6 may keep a different one of the pair."""
    assert not np.any(np.abs(scores - thr) < eps_score), "a score next to the threshold"
    n = len(scores)
    x1 = np.maximum(boxes[:, None, 0], boxes[None, :, 0])
    y1 = np.maximum(boxes[:, None, 1], boxes[None, :, 1])
    x2 = np.minimum(boxes[:, None, 2], boxes[None, :, 2])
    y2 = np.minimum(boxes[:, None, 3], boxes[None, :, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    iou = inter / (area[:, None] + area[None, :] - inter)
    same = (classes[:, None] == classes[None, :]) & ~np.eye(n, dtype=bool)
    assert not np.any(same & (np.abs(iou - iou_thr) < eps_iou)), "an IoU next to the NMS threshold"
    return int(R.near_ties(boxes, scores, classes, iou_thr, eps_score).sum())


def candidates(anc, reg, cls, thr):
    """Per image: the anchors whose class max passes thr, their decoded boxes on the canvas, scores and classes."""
    out = []
    for i in range(reg.shape[0]):
        idx = np.nonzero(cls[i].max(1) > np.float32(thr))[0]
        r = np.zeros_like(reg[i])
        r[idx] = reg[i][idx]
        c = np.zeros_like(cls[i])
        c[idx] = cls[i][idx]
        bx = R.decode(anc, r)[idx]
        out.append((idx, bx, cls[i][idx].max(1), cls[i][idx].argmax(1)))
    return out


def main():
    Det, U = _import_reference()
    torch.manual_seed(0)
    out = {}
    imgs = R.images()
    chw = [im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in imgs]
    for cc in (0, 3):
        m = Det(compound_coef=cc, num_classes=1, ratios=[(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)],
                scales=[2 ** 0, 2 ** (1.0 / 3.0), 2 ** (2.0 / 3.0)], threshold=0.5, iou_threshold=0.5).eval()
        sd = m.state_dict()
        layout = "\n".join(f"{k} {','.join(map(str, v.shape))}" for k, v in sd.items())
        out[f"d{cc}_layout"] = np.frombuffer(layout.encode(), np.uint8)
        m.load_state_dict(R.synth_state_dict({k: tuple(v.shape) for k, v in sd.items()}), strict=True)
        with torch.no_grad():
            if cc == 0:
                _, canvas, metas = U.preprocess(chw, max_size=512)
                feats, reg, cls, anc = m(chw, postprocess=False)
                p345 = m.backbone_net(canvas)[1:]
                for i, t in enumerate(p345):
                    assert torch.isfinite(t).all() and t.abs().max() < 1e3
                    out[f"p{i + 3}_s"], out[f"p{i + 3}_stats"] = strided(t), stats(t)
                for i, t in enumerate(feats):
                    assert torch.isfinite(t).all() and t.abs().max() < 1e3
                    out[f"f{i}_s"], out[f"f{i}_stats"] = strided(t), stats(t)
                out["canvas_s"] = canvas[:, :, ::8, ::8].numpy()
                out["cls"] = cls.numpy()
                cand = candidates(anc[0].numpy(), reg.numpy(), cls.numpy(), LO_THR)
                for i, (idx, _, _, _) in enumerate(cand):   # the regression rows of every anchor above lo_thr
                    out[f"cand{i}_idx"], out[f"cand{i}_reg"] = idx.astype(np.int32), reg[i, idx].numpy()
                out["reg_stats"] = stats(reg)
                out["anchors_sum"] = np.array([anc.double().sum().item(), (anc.double() * torch.arange(anc.shape[1])[None, :, None]).sum().item()])
                passing = (cls.max(2)[0] > 0.5).sum(1)
                assert all(50 <= int(n) <= 3000 for n in passing), passing
                dets = m(chw)
                raw = U.postprocess(canvas, anc, reg, cls, U.BBoxTransform(), U.ClipBoxes(), threshold=0.5, iou_threshold=0.5)
                ties = [check_margins(bx, sc, cl, 0.5, 0.5) for _, bx, sc, cl in candidates(anc[0].numpy(), reg.numpy(), cls.numpy(), 0.5)]
                for i, d in enumerate(dets):
                    out[f"det{i}_boxes"], out[f"det{i}_labels"], out[f"det{i}_scores"] = (d["boxes"].numpy(), d["labels"].numpy(),
                                                                                       d["scores"].numpy())
                    assert len(d["scores"]) > 0
                lo = U.postprocess(canvas, anc, reg, cls, U.BBoxTransform(), U.ClipBoxes(), threshold=LO_THR, iou_threshold=0.5)
                nlo = (cls.max(2)[0] > LO_THR).sum(1)
                assert int(nlo[0]) > 4096, nlo
                assert not np.any(np.abs(cls.numpy().max(2) - LO_THR) < 1e-5), "a score next to lo_thr"
                out["lo_thr"] = np.float64(LO_THR)
                for i, r in enumerate(lo):
                    out[f"lo{i}_rois"], out[f"lo{i}_class_ids"], out[f"lo{i}_scores"] = r["rois"], r["class_ids"], r["scores"]
                out["metas"] = np.array([mm for mm in metas], np.int64)
                print("D0: passing", passing.tolist(), "kept", [len(d["scores"]) for d in dets], "low-thr candidates", nlo.tolist(),
                      "kept", [len(r["scores"]) for r in lo],
                      "near-tied candidates at 0.5", ties)
            else:
                feats, reg, cls, _ = m(chw[:1], postprocess=False)
                out["d3_reg_stats"], out["d3_cls_stats"] = stats(reg), stats(cls)
                out["d3_f_stats"] = np.stack([stats(t) for t in feats])
    path = os.path.join(OUT, "g15_effdet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
