"""Pose scoring on the MI355X: the device counterparts of ``evaluate.rescore_and_nms`` (``lib/metrics.py:211-262`` with
``lib/nms.py``) and ``evaluate.oks_ap`` (the published ``COCOeval(..., "keypoints")``), which the evaluation of
``src/03_evaluate.py`` runs after the network.

  * ``stlpose::pose_rescore_nms`` (per image: score = box score x mean confidence of the confident joints, greedy OKS suppression),
  * ``stlpose::oks_ap_match`` (evaluateImg: per image sort, fp64 OKS tile, greedy match for 10 thresholds x 3 area ranges),
  * one global stable score order (``torch.sort(stable=True)`` over all slots),
  * ``stlpose::box_ap_accumulate`` (accumulate: it reads match / ignore bits, ranks and counts only, so it serves keypoints unchanged),

and the 10 means of ``summarize`` on the host.  Keypoints and scores are float64, as the host path holds them.

Exactness.  Scores are those of the host bit for bit (the mean confidence is summed in numpy's order; ``mean_order="reference"``
sums it as the reference's loop does and gives the reference's scores bit for bit, one ulp away for some persons).  An OKS value is the host's
up to the device's fp64 ``exp`` (below 1e-13), and OKS values are only compared -- with a threshold, and with each other for the
best match -- so kept lists, precision and recall equal the host's whenever no such comparison is closer than that
(``tests/keypoint_eval_ref.py`` measures the margins).  The rescoring + NMS half is pinned by the reference fixtures G7 and G12;
the AP half restates pycocotools like ``oks_ap`` does: **parity unpinned**.

Caps: ``capi.POSE_NMS_MAX`` persons per image for the NMS, ``capi.BOX_MAX`` results and ``capi.BOX_AP_GT_MAX`` ground truths per
image for AP, 17 joints.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import capi
from .coco_tables import REC_THRS, device_of, image_rows, match_and_accumulate, mean_valid as _mean, offsets_of, take_images  # noqa: F401
from .evaluate import COCO_SIGMAS

OKS_THRS = np.linspace(.5, 0.95, 10)
AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))   # all, medium, large
STAT_NAMES = ("AP", "AP50", "AP75", "AP(M)", "AP(L)", "AR", "AR50", "AR75", "AR(M)", "AR(L)")


def _sigmas(sigmas) -> List[float]:
    s = COCO_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64).reshape(-1)
    if len(s) != capi.POSE_JOINTS:
        raise ValueError(f"keypoint scoring on the device is built for {capi.POSE_JOINTS} joints, got {len(s)} sigmas; "
                         "evaluate.oks_ap on the host takes any count")
    return [float(v) for v in s]


class PoseResults:
    """The persons ``rescore_and_nms`` keeps, as device tables: ``keypoints`` float64 [N, 17, 3], ``scores`` float64 [N],
    ``image_ids`` int64 [I] (numpy, in order of first appearance) and ``offsets`` int64 [I + 1] (numpy): image i owns rows
    offsets[i] .. offsets[i+1]-1, in NMS order."""

    def __init__(self, keypoints: torch.Tensor, scores: torch.Tensor, image_ids: np.ndarray, offsets: np.ndarray):
        self.keypoints, self.scores = keypoints, scores
        self.image_ids, self.offsets = np.asarray(image_ids, np.int64), np.asarray(offsets, np.int64)
        if tuple(keypoints.shape[1:]) != (capi.POSE_JOINTS, 3) or scores.shape != keypoints.shape[:1]:
            raise ValueError(f"PoseResults: keypoints {tuple(keypoints.shape)}, scores {tuple(scores.shape)}")
        if len(self.offsets) != len(self.image_ids) + 1 or int(self.offsets[-1]) != keypoints.shape[0]:
            raise ValueError(f"PoseResults: {len(self.image_ids)} images, offsets {self.offsets[-5:]}, {keypoints.shape[0]} persons")

    def __len__(self) -> int:
        return int(self.keypoints.shape[0])

    def to_list(self) -> List[dict]:
        """The list of COCO result dicts ``rescore_and_nms`` returns, in the same order."""
        kp = self.keypoints.detach().cpu().numpy().reshape(len(self), capi.POSE_JOINTS * 3).tolist()
        sc = self.scores.detach().cpu().numpy().tolist()
        ids = np.repeat(self.image_ids, np.diff(self.offsets)).tolist()
        return [dict(image_id=int(i), category_id=1, keypoints=k, score=s) for i, k, s in zip(ids, kp, sc)]

    @classmethod
    def from_list(cls, results: Sequence[dict], device=None) -> "PoseResults":
        """A result list whose images lie in one run each (what ``to_list`` gives) as tables."""
        dev = device_of(device)
        ids = np.asarray([r["image_id"] for r in results], np.int64)
        start = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]])) if len(ids) else np.zeros(0, np.int64)
        if len(np.unique(ids[start])) != len(start):
            raise ValueError("PoseResults.from_list: the results of an image must be adjacent")
        kp = np.asarray([r["keypoints"] for r in results], np.float64).reshape(-1, capi.POSE_JOINTS, 3)
        sc = np.asarray([r["score"] for r in results], np.float64)
        return cls(torch.from_numpy(kp).to(dev), torch.from_numpy(sc).to(dev), ids[start], np.concatenate([start, [len(ids)]]))


def rescore_and_nms_device(all_preds, all_boxes, image_ids: Sequence, in_vis_thr: float = 0.2, oks_thr: float = 0.9,
                           device=None, mean_order: str = "numpy") -> PoseResults:
    """``evaluate.rescore_and_nms`` on the device.  all_preds [P, 17, 3] float32 or float64 (x, y, confidence), all_boxes [P, 6]
    (centre, scale, area, box score), numpy or tensors; image_ids: one id per person, the persons of an image anywhere in the list.
    mean_order: how the confident joints are summed.  ``"numpy"``: as ``conf[good].mean()`` sums them, so the scores are those of
    ``evaluate.rescore_and_nms`` bit for bit; ``"reference"``: one after the other, as the loop of ``lib/metrics.py:242-250`` does,
    so the scores are the reference's bit for bit (fixture G12).  The two differ by one ulp for some persons with eight or more
    confident joints."""
    if mean_order not in capi.POSE_SUM_ORDER:
        raise ValueError(f"rescore_and_nms_device: mean_order {mean_order!r} ('numpy' or 'reference')")
    from . import ops  # noqa: F401  (registers the stlpose:: ops)
    dev = device_of(device)
    preds = torch.as_tensor(all_preds)
    if preds.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"rescore_and_nms_device: all_preds must be float32 or float64, got {preds.dtype}")
    boxes = torch.as_tensor(all_boxes).to(torch.float64)
    ids = np.asarray(image_ids, np.int64).reshape(-1)
    if preds.dim() != 3 or tuple(preds.shape[1:]) != (capi.POSE_JOINTS, 3) or tuple(boxes.shape) != (preds.shape[0], 6) \
            or len(ids) != preds.shape[0]:
        raise ValueError(f"rescore_and_nms_device: all_preds {tuple(preds.shape)} ([P, {capi.POSE_JOINTS}, 3]), all_boxes "
                         f"{tuple(boxes.shape)} ([P, 6]), {len(ids)} image ids")
    # the persons grouped by image, images in order of first appearance, input order within an image
    uniq, first, inv, cnt = np.unique(ids, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(first, kind="stable")
    rank_of = np.empty(len(uniq), np.int64)
    rank_of[by_first] = np.arange(len(uniq))
    perm = np.argsort(rank_of[inv.reshape(-1)], kind="stable")
    img_ids, cnt = uniq[by_first], cnt[by_first]
    offsets = offsets_of(cnt)
    if len(cnt) and int(cnt.max()) > capi.POSE_NMS_MAX:
        w = int(cnt.argmax())
        raise ValueError(f"image_id {int(img_ids[w])}: {int(cnt[w])} persons; the cap of the device NMS is {capi.POSE_NMS_MAX} "
                         "(STL_POSE_NMS_MAX) per image")
    sorted_already = bool((perm == np.arange(len(perm))).all())
    preds, boxes = preds.to(dev), boxes.to(dev)
    if not sorted_already:
        p = torch.from_numpy(perm).to(dev)
        preds, boxes = preds[p], boxes[p]
    score, keep, count = torch.ops.stlpose.pose_rescore_nms(preds, boxes, torch.from_numpy(offsets), float(in_vis_thr), float(oks_thr),
                                                            _sigmas(None), mean_order == "reference")
    kept = count.cpu().numpy().astype(np.int64)
    rows = (keep.long() + torch.from_numpy(np.repeat(offsets[:-1], cnt)).to(dev))[keep >= 0]
    return PoseResults(preds[rows].to(torch.float64), score[rows], img_ids, offsets_of(kept))


class KeypointGroundTruth:
    """COCO person annotations as a ragged device table, images ascending by id: uploaded once, sliced per evaluation."""

    def __init__(self, annotations: Sequence[dict], device=None):
        anns = sorted(annotations, key=lambda a: a["image_id"])   # stable: annotation order within an image
        ids = np.asarray([a["image_id"] for a in anns], np.int64)
        self.img_ids, self.counts = np.unique(ids, return_counts=True)
        self.device = dev = device_of(device)
        j = capi.POSE_JOINTS
        for a in anns:
            if len(a["keypoints"]) != 3 * j:
                raise ValueError(f"KeypointGroundTruth: annotation of image {a['image_id']} has {len(a['keypoints'])} keypoint values "
                                 f"({3 * j} for {j} joints)")
        self.kpts = torch.from_numpy(np.asarray([a["keypoints"] for a in anns], np.float64).reshape(-1, j, 3)).to(dev)
        self.area = torch.from_numpy(np.asarray([a["area"] for a in anns], np.float64)).to(dev)
        self.bbox = torch.from_numpy(np.asarray([a["bbox"] for a in anns], np.float64).reshape(-1, 4)).to(dev)
        self.crowd = torch.from_numpy(np.asarray([bool(a.get("iscrowd", 0)) for a in anns], np.uint8)).to(dev)
        self.numkp = torch.from_numpy(np.asarray([int(a.get("num_keypoints", 1)) for a in anns], np.int32)).to(dev)

    def select(self, img_ids: np.ndarray):
        """The rows of the given images (ascending ids; an image without annotations has none): tensors and offsets.  For every
        image of the table, in order, these are the stored tables themselves, not copies."""
        tables, offsets = take_images((self.kpts, self.area, self.bbox, self.crowd, self.numkp), self.img_ids, self.counts, img_ids,
                                      self.device)
        return (*tables, offsets)


class KeypointEval:
    """What ``COCOeval`` holds after accumulate / summarize for "keypoints": ``precision`` [T, R, A], ``recall`` [T, A] (numpy, -1
    where an area range has no ground truth to find) and ``stats`` [10]."""

    def __init__(self, precision: np.ndarray, recall: np.ndarray):
        self.precision, self.recall = precision, recall
        self.stats = summarize(precision, recall)


def summarize(precision: np.ndarray, recall: np.ndarray) -> np.ndarray:
    """The 10 numbers of ``STAT_NAMES`` with the slicing and the mean of ``oks_ap``."""
    t50, t75 = 0, 5
    return np.array([_mean(precision[:, :, 0]), _mean(precision[t50, :, 0]), _mean(precision[t75, :, 0]),
                     _mean(precision[:, :, 1]), _mean(precision[:, :, 2]),
                     _mean(recall[:, 0]), _mean(recall[t50:t50 + 1, 0]), _mean(recall[t75:t75 + 1, 0]),
                     _mean(recall[:, 1]), _mean(recall[:, 2])])


def evaluate_tables(kpts, scores, area, det_offsets, gt: tuple, sigmas: Sequence[float], max_dets: int, img_ids=None):
    """match + order + accumulate on the device for ragged tables whose images are in ascending id order.  kpts float64 [N, 17, 3],
    scores float64 [N], area float64 [N] or None, det_offsets int64 [I + 1] (CPU); gt = (kpts, area, bbox, crowd, numkp, offsets).
    Returns (precision [T, R, A], recall [T, A]) as device tensors.  img_ids: an exceeded cap is reported with the image's id."""
    gk, ga, gb, gc, gn, goff = gt
    precision, recall = match_and_accumulate(lambda: torch.ops.stlpose.oks_ap_match(
        kpts, scores, area, det_offsets, gk, ga, gb, gc, gn, goff, [float(t) for t in OKS_THRS],
        [float(v) for r in AREA_RANGES for v in r], [float(s) for s in sigmas]), 1, len(OKS_THRS), [int(max_dets)], img_ids)
    return precision[:, :, 0, :, 0], recall[:, 0, :, 0]


def keypoint_ap_tables(gt_annotations: Union[Sequence[dict], KeypointGroundTruth], results: Union[Sequence[dict], PoseResults],
                  img_ids: Optional[Sequence[int]] = None, sigmas=None, max_dets: int = 20, device=None) -> KeypointEval:
    """``keypoint_ap`` with the tables its numbers are read from: ``.precision`` [10, 101, 3], ``.recall`` [10, 3], ``.stats`` [10]."""
    sg = _sigmas(sigmas)
    if not 1 <= int(max_dets) <= capi.OKS_AP_DETS:
        raise ValueError(f"keypoint AP: max_dets must be in 1 .. {capi.OKS_AP_DETS} (STL_OKS_AP_DETS), got {max_dets}")
    table = gt_annotations if isinstance(gt_annotations, KeypointGroundTruth) else None
    dev = table.device if table is not None and device is None else device_of(device)
    j = capi.POSE_JOINTS
    if isinstance(results, PoseResults):
        by_id = np.argsort(results.image_ids, kind="stable")
        rid_img, rcnt, rstart = results.image_ids[by_id], np.diff(results.offsets)[by_id], results.offsets[:-1][by_id]
        if len(np.unique(rid_img)) != len(rid_img):
            raise ValueError("keypoint AP: a PoseResults names an image twice")
    else:
        results = sorted(results, key=lambda r: r["image_id"])    # stable: result order within an image
        rid = np.asarray([r["image_id"] for r in results], np.int64)
        rid_img, rcnt = np.unique(rid, return_counts=True)
        rstart = offsets_of(rcnt)[:-1]
    gt_ids = table.img_ids if table is not None else np.asarray(sorted({int(a["image_id"]) for a in gt_annotations}), np.int64)
    ids = np.union1d(gt_ids, rid_img) if img_ids is None else np.asarray(sorted(set(int(i) for i in img_ids)), np.int64)
    if table is None:
        table = KeypointGroundTruth(gt_annotations, device=dev)
    # the results of the scored images, images ascending by id
    rows, offsets = image_rows(rid_img, rcnt, rstart, ids)
    if isinstance(results, PoseResults):
        r = torch.from_numpy(rows).to(results.keypoints.device)
        kpts, scores, area = results.keypoints[r].to(dev), results.scores[r].to(dev), None
    else:
        res = [results[i] for i in rows]
        for r in res:
            if len(r["keypoints"]) != 3 * j:
                raise ValueError(f"keypoint AP: a result of image {r['image_id']} has {len(r['keypoints'])} keypoint values ({3 * j} for "
                                 f"{j} joints)")
        kpts = torch.from_numpy(np.asarray([r["keypoints"] for r in res], np.float64).reshape(-1, j, 3)).to(dev)
        scores = torch.from_numpy(np.asarray([r["score"] for r in res], np.float64)).to(dev)
        given = np.asarray(["area" in r for r in res], bool)
        area = None
        if given.any():   # COCO.loadRes for keypoints: a result without an area gets that of its keypoints' bounding box
            a = torch.from_numpy(np.asarray([r.get("area", 0.0) for r in res], np.float64)).to(dev)
            if not given.all():
                x, y = kpts[:, :, 0], kpts[:, :, 1]
                derived = (x.max(1).values - x.min(1).values) * (y.max(1).values - y.min(1).values)
                a = torch.where(torch.from_numpy(given).to(dev), a, derived)
            area = a
    precision, recall = evaluate_tables(kpts, scores, area, torch.from_numpy(offsets), table.select(ids), sg, int(max_dets),
                                        img_ids=ids)
    return KeypointEval(np.ascontiguousarray(precision.cpu().numpy()), np.ascontiguousarray(recall.cpu().numpy()))


def keypoint_ap(gt_annotations: Union[Sequence[dict], KeypointGroundTruth], results: Union[Sequence[dict], PoseResults],
                img_ids: Optional[Sequence[int]] = None, sigmas=None, max_dets: int = 20, device=None) -> np.ndarray:
    """Keypoint AP/AR with COCOeval semantics on the device, the counterpart of ``evaluate.oks_ap``.  gt_annotations: COCO person
    annotations (image_id, keypoints[51], num_keypoints, area, bbox, iscrowd) or a ``KeypointGroundTruth`` built once; results: COCO
    result dicts (image_id, keypoints[51], score, optionally area) or a ``PoseResults``.  img_ids: the images to score (default:
    every image either side names); results of other images are dropped.  Returns the 10 numbers of COCOeval.stats for keypoints:
    AP, AP50, AP75, AP(M), AP(L), AR, AR50, AR75, AR(M), AR(L)."""
    return keypoint_ap_tables(gt_annotations, results, img_ids, sigmas, max_dets, device).stats
