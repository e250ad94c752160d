"""Top-down pose extraction: person boxes -> crops -> HRNet -> poses in image and crop coordinates.

The glue of the reference's 04_evaluate_vases_qualitatively.py:184-250 (detector boxes -> ``bbox_filtering`` ->
``TransformDetection`` crops -> HRNet -> 4x bilinear upsample -> argmax -> ``create_pose_entries``, and ``get_final_preds_hrnet``
for the full-image poses) and 05_create_archdata_retrieval_db.py:114-171 (dataset crops -> flip-test forward -> the same decode
-> the retrieval database dict that ``fit_knn_structure`` takes).  Every step runs on the device: one ``box_select`` launch for
the boxes of all images, one ``affine_crop`` for all persons, HRNet in fixed chunks, ``final_preds`` and the fused
``heatmap_resize_argmax``; only 17 x 3 numbers per person and decode reach the host.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)
from .augment import IMAGENET_MEAN, IMAGENET_STD, affine_matrices, crop_batch
from .bounding_box import select_boxes
from .inference import forward_pass
from .pose_parsing import create_pose_entries


def _image(img, dev) -> torch.Tensor:
    t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"images must be uint8 HWC RGB, got {t.dtype} {tuple(t.shape)}")
    return t.to(dev)


def _ref_scales(scales) -> np.ndarray:
    """float32 scales -> the float64 scales whose box width scale * 200 is the reference's: its get_affine_transform rounds
    scale * 200 to float32 (lib/transforms.py:206)."""
    return (np.asarray(scales, np.float32) * np.float32(200)).astype(np.float64) / 200.0


class TransformDetection:
    """lib/transforms.py:14-82: the person crop of each box (x1, y1, x2, y2), centred on the box, widened to the crop's aspect
    ratio and by 1.25.  The crops come from augment.crop_batch (one launch for all boxes; rot = 0, no flip) as a device tensor
    [n, 3, det_height, det_width]; normalize=True (default) gives the network's input (ToTensor + ImageNet Normalize, what the
    reference's caller applies to its crops), normalize=False the ToTensor scale [0, 1] -- the reference returns 0..255 pixels.
    img: one uint8 HWC RGB image (tensor or array)."""

    def __init__(self, det_width=192, det_height=256):
        self.det_width, self.det_height = det_width, det_height
        self.image_size = np.array([det_width, det_height])
        self.aspect_ratio = det_width * 1.0 / det_height
        self.pixel_std = 200

    def _coords2cs(self, coords):
        """One box -> (center, scale), float32 like the reference."""
        c, s = self.coords2cs(np.asarray(coords, np.float32).reshape(1, 4))
        return c[0], s[0]

    def coords2cs(self, coords):
        """All boxes [n, 4] at once: the reference's _coords2cs restated in float32."""
        b = np.asarray(coords, np.float32).reshape(-1, 4)
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        center = np.stack([b[:, 0] + w * np.float32(0.5), b[:, 1] + h * np.float32(0.5)], 1)
        ar = np.float32(self.aspect_ratio)
        wider, taller = w > ar * h, w < ar * h
        h2 = np.where(wider, w * np.float32(1.0) / ar, h)
        w2 = np.where(~wider & taller, h * ar, w)
        scale = np.stack([w2 * np.float32(1.0) / np.float32(self.pixel_std), h2 * np.float32(1.0) / np.float32(self.pixel_std)], 1)
        scale = np.where((center[:, 0] != -1)[:, None], scale * np.float32(1.25), scale).astype(np.float32)
        return center.astype(np.float32), scale

    def matrices(self, centers, scales) -> np.ndarray:
        """The [n, 2, 3] crop matrices the reference's get_affine_transform gives for these centers / scales."""
        box = _ref_scales(scales)
        return affine_matrices(np.asarray(centers, np.float64), box, np.zeros(len(box)), (self.det_width, self.det_height))

    def crops(self, images: Sequence[torch.Tensor], centers, scales, normalize=True) -> torch.Tensor:
        """Crop person k out of images[k] (device uint8 HWC tensors) for all k in one launch."""
        n = len(images)
        out, _ = crop_batch(images, centers, _ref_scales(scales), np.zeros(n), np.zeros(n, bool), (self.det_width, self.det_height),
                            normalize=normalize, device=images[0].device if n else None)
        return out

    def __call__(self, img, list_coords, normalize=True, device=None):
        centers, scales = self.coords2cs(list_coords)
        if len(centers) == 0:
            return torch.zeros(0, 3, self.det_height, self.det_width), centers, scales
        im = _image(img, torch.device(device or "cuda"))
        return self.crops([im] * len(centers), centers, scales, normalize), centers, scales


class PoseExtractor:
    """Poses of the persons in a batch of images, from any detector's boxes (04_evaluate_vases_qualitatively.py:184-250).

    extractor(images, boxes, scores=None, labels=None, label=1, det_thr=0.7, nms_thr=None) -> one dict per image.  images: uint8
    HWC RGB (tensors or arrays); boxes[i] [n_i, 4] (x1, y1, x2, y2); with scores, a box is kept when label matches (if labels
    are given) and score > det_thr, then (nms_thr) greedy NMS -- one box_select launch for all images.  Each dict holds "boxes",
    "scores" (the kept ones, in detector order, or score order after NMS), "center", "scale", "keypoints" [n, 17, 3] (image
    coordinates from get_final_preds_hrnet, and the maxval), "crop_keypoints" [n, 17, 3] (the 4x-upsampled argmax in crop
    coordinates, and its maxval), "pose_entries" and "all_keypoints" (create_pose_entries of the image-coordinate poses with
    columns swapped, 04's full-image format).

    All persons of all images go through the network in chunks of `batch`, the last one zero-padded, so the model builds one
    plan per (batch, resolution, dtype), whatever the person counts.  flip=True runs forward_pass's flip test."""

    def __init__(self, model, image_size=(192, 256), flip=False, batch=32, keypoint_thr=0.1):
        self.model, self.flip, self.batch, self.keypoint_thr = model, flip, int(batch), keypoint_thr
        self.transform = TransformDetection(det_width=int(image_size[0]), det_height=int(image_size[1]))

    def heatmaps(self, crops: torch.Tensor) -> torch.Tensor:
        """The network on [P, 3, H, W] crops in chunks of `batch` (the last zero-padded) -> [P, J, h, w] heat maps."""
        outs = []
        for a in range(0, crops.shape[0], self.batch):
            chunk = crops[a:a + self.batch]
            n = chunk.shape[0]
            if n < self.batch:
                chunk = torch.cat([chunk, chunk.new_zeros(self.batch - n, *chunk.shape[1:])])
            with torch.no_grad():
                outs.append(forward_pass(self.model, chunk, flip=self.flip)[:n])
        return torch.cat(outs)

    def __call__(self, images, boxes, scores=None, labels=None, label=1, det_thr=0.7, nms_thr=None) -> List[Dict]:
        if len(images) != len(boxes):
            raise ValueError(f"{len(images)} images but {len(boxes)} box lists")
        bs = [np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float32).reshape(-1, 4) for b in boxes]
        ss = None if scores is None else [np.asarray(s.detach().cpu() if torch.is_tensor(s) else s, np.float32).reshape(-1) for s in scores]
        if ss is not None and sum(len(b) for b in bs):
            kept = select_boxes(bs, ss, labels, label=int(label), score_thr=float(np.float32(det_thr)),
                                iou_thr=-1.0 if nms_thr is None else float(nms_thr))
        else:
            kept = [np.arange(len(b)) for b in bs]
        kb = [b[k] for b, k in zip(bs, kept)]
        ks = [s[k] for s, k in zip(ss, kept)] if ss is not None else [np.ones(len(k), np.float32) for k in kept]
        counts = [len(b) for b in kb]
        total = sum(counts)
        centers, scales = self.transform.coords2cs(np.concatenate(kb) if total else np.zeros((0, 4), np.float32))
        res = [dict(boxes=b, scores=s) for b, s in zip(kb, ks)]
        if total:
            dev = torch.device("cuda")
            src = [_image(im, dev) if n else None for im, n in zip(images, counts)]
            crops = self.transform.crops([src[i] for i, n in enumerate(counts) for _ in range(n)], centers, scales)
            hm = self.heatmaps(crops)
            c, s = torch.from_numpy(centers).to(hm.device), torch.from_numpy(scales).to(hm.device)
            preds, mx = torch.ops.stlpose.final_preds(hm, c, s)
            _, cmx, cpreds = torch.ops.stlpose.heatmap_resize_argmax(hm.float(), self.transform.det_height, self.transform.det_width)
            kp = torch.cat([preds, mx], 2).cpu().numpy()
            ckp = torch.cat([cpreds, cmx[..., None]], 2).cpu().numpy()
        j = 17
        a = 0
        for r, n in zip(res, counts):
            r["center"], r["scale"] = centers[a:a + n], scales[a:a + n]
            if n:
                r["keypoints"], r["crop_keypoints"] = kp[a:a + n], ckp[a:a + n]
                entries, all_kp = create_pose_entries(r["keypoints"][..., :2], r["keypoints"][..., 2:], thr=self.keypoint_thr)
                r["pose_entries"], r["all_keypoints"] = entries, all_kp[:, [1, 0, 2, 3]]
            else:
                r["keypoints"] = r["crop_keypoints"] = np.zeros((0, j, 3), np.float32)
                r["pose_entries"], r["all_keypoints"] = [], np.zeros((0, 4))
            a += n
        return res

    # -- from device tables
    def person_rows(self, detections, label=1, det_thr=0.7, nms_thr=None):
        """The person rows of a ``Detections`` on the device (``stlpose::person_boxes``): bbox_filtering's label / score test, the
        optional NMS, coords2cs and the crop matrices.  Returns (n, img int32 [n], boxes [n, 4], scores [n], center [n, 2], scale
        [n, 2], minv [n, 6]) with the tensors on the device; reading n, the person count, is the one wait."""
        t = self.transform
        img, boxes, scores, center, scale, minv, total = torch.ops.stlpose.person_boxes(
            detections.boxes, detections.scores, detections.labels, detections.count, int(label), float(np.float32(det_thr)),
            -1.0 if nms_thr is None else float(nms_thr), float(np.float32(t.aspect_ratio)), t.det_width, t.det_height)
        n = int(total.item())
        if n < 0:
            raise ValueError(f"PoseExtractor: image {-n - 1} of the batch has more candidates than the device path holds "
                             f"({capi.BOX_MAX}, STL_BOX_MAX); raise the detector's threshold or use the host pipeline")
        return n, img[:n], boxes[:n], scores[:n], center[:n], scale[:n], minv[:n]

    def from_detections(self, images, detections, label=1, det_thr=0.7, nms_thr=None) -> List[Dict]:
        """``__call__`` for a detector's device tables (``forward(output="device")``): the boxes never visit the host.  The person
        count is read once, to size the chunk loop; then affine_crop, the network, final_preds and heatmap_resize_argmax run on
        device tensors and one copy brings boxes, scores, centers, scales and poses back.  The same dicts as ``__call__``."""
        if len(images) != len(detections):
            raise ValueError(f"{len(images)} images but detections of {len(detections)}")
        dev = detections.device
        n, img, boxes, scores, center, scale, minv = self.person_rows(detections, label, det_thr, nms_thr)
        j = 17
        host = np.zeros((0, 10 + 6 * j), np.float32)
        if n:
            src = [_image(im, dev) for im in images]
            sizes = [s.numel() for s in src]
            offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).to(dev, non_blocking=True)
            hw = torch.tensor([[s.shape[0], s.shape[1]] for s in src], dtype=torch.int32).to(dev, non_blocking=True)
            which = img.long()
            mean, std = torch.tensor(IMAGENET_MEAN, device=dev), torch.tensor(IMAGENET_STD, device=dev)
            crops = torch.ops.stlpose.affine_crop(torch.cat([s.reshape(-1) for s in src]), offs[which], hw[which], minv,
                                                  torch.zeros(n, dtype=torch.int32, device=dev), self.transform.det_height,
                                                  self.transform.det_width, mean, std)
            hm = self.heatmaps(crops)
            preds, mx = torch.ops.stlpose.final_preds(hm, center, scale)
            _, cmx, cpreds = torch.ops.stlpose.heatmap_resize_argmax(hm.float(), self.transform.det_height, self.transform.det_width)
            j = preds.shape[1]
            host = torch.cat([img.float()[:, None], boxes, scores[:, None], center, scale, torch.cat([preds, mx], 2).reshape(n, -1),
                              torch.cat([cpreds, cmx[..., None]], 2).reshape(n, -1)], 1).cpu().numpy()
        counts = np.bincount(host[:, 0].astype(np.int64), minlength=len(images))
        res, a = [], 0
        for c in counts.tolist():
            rows = host[a:a + c]
            r = dict(boxes=rows[:, 1:5].copy(), scores=rows[:, 5].copy(), center=rows[:, 6:8].copy(), scale=rows[:, 8:10].copy())
            if c:
                r["keypoints"] = rows[:, 10:10 + 3 * j].reshape(c, j, 3).copy()
                r["crop_keypoints"] = rows[:, 10 + 3 * j:].reshape(c, j, 3).copy()
                entries, all_kp = create_pose_entries(r["keypoints"][..., :2], r["keypoints"][..., 2:], thr=self.keypoint_thr)
                r["pose_entries"], r["all_keypoints"] = entries, all_kp[:, [1, 0, 2, 3]]
            else:
                r["keypoints"] = r["crop_keypoints"] = np.zeros((0, j, 3), np.float32)
                r["pose_entries"], r["all_keypoints"] = [], np.zeros((0, 4))
            res.append(r)
            a += c
        return res


def extract_retrieval_db(model, loader, flip=True, keypoint_thr=0.1, device=None) -> Dict[str, Dict]:
    """05_create_archdata_retrieval_db.py:114-171 (extract_retrieval_dataset): for every loader batch (imgs, _, _, metadata) with
    metadata "center", "scale", "image", "character_name", the flip-test forward, the fused 256 x 192 decode and one entry per
    person: {"img", "joints" [17, 3] = (x, y, vis), "center" [1, 2], "scale" [1, 2], "character_name"} under "img_<k>" -- the
    dict fit_knn_structure takes.  For a loader batch of 1 this is the reference's entry exactly; for larger batches the reference
    puts all persons of the batch into one entry (joints [B * 17, 3], the batch's centers), here every person gets its own."""
    dev = torch.device(device or "cuda")
    db: Dict[str, Dict] = {}
    for imgs, _, _, meta in loader:
        hm = forward_pass(model, imgs.to(dev).float(), flip=flip)
        _, mx, preds = torch.ops.stlpose.heatmap_resize_argmax(hm.float(), 256, 192)
        preds, mx = preds.cpu().numpy(), mx.cpu().numpy()
        centers, scales = np.asarray(meta["center"], np.float32), np.asarray(meta["scale"], np.float32)
        for p in range(preds.shape[0]):
            _, all_kp = create_pose_entries(preds[p:p + 1], mx[p:p + 1, :, None], thr=keypoint_thr)
            db[f"img_{len(db)}"] = {"img": meta["image"][p], "joints": torch.Tensor(all_kp[:, [0, 1, 3]]).float(),
                                    "center": torch.Tensor(centers[p:p + 1]).float(), "scale": torch.Tensor(scales[p:p + 1]).float(),
                                    "character_name": meta["character_name"][p]}
    return db


def detect_poses(detector, extractor: PoseExtractor, images, detector_thr=0.7, nms_thr=None, pipeline="host") -> List[Dict]:
    """04_evaluate_vases_qualitatively.py:184-250 from raw images: uint8 HWC RGB images (tensors or arrays) -> the EfficientDet
    detector (preprocessed on the device from the same device images) -> bbox_filtering's person boxes (label 1, score >
    detector_thr) -> ``extractor``.  Returns the extractor's dicts; only the detector's kept boxes and the poses reach the host.
    pipeline="device": the detections stay device tables from the heads to the crops (``PoseExtractor.from_detections``); the
    host reads the person count and, at the end, the results."""
    if pipeline not in ("host", "device"):
        raise ValueError(f"detect_poses: pipeline {pipeline!r} (one of 'host', 'device')")
    dev = torch.device("cuda", torch.cuda.current_device())
    src = [_image(im, dev) for im in images]
    if not src:
        return []
    p, metas = detector.run_raw(src, 0, dev)
    if pipeline == "device":
        dets = detector.detect(p, metas, detector.threshold, detector.iou_threshold, output="device")
        return extractor.from_detections(src, dets, label=1, det_thr=detector_thr, nms_thr=nms_thr)
    dets = detector.detect(p, metas, detector.threshold, detector.iou_threshold)
    return extractor(src, [d["boxes"].reshape(-1, 4) for d in dets], [d["scores"] for d in dets], [d["labels"].long() for d in dets],
                     label=1, det_thr=detector_thr, nms_thr=nms_thr)
