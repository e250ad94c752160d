"""Detector validation on the MI355X: COCO box AP, the counterpart of the reference's ``CocoEvaluator(coco, ["bbox"])``
(``02_train_faster_rcnn.py:241-280``, ``03_evaluate_faster_rcnn.py:119-184``).

The reference delegates to ``pycocotools.cocoeval.COCOeval(..., "bbox")``, a third-party dependency that is neither vendored in the
reference tree nor installed here.  This module restates its published algorithm -- **parity unpinned**, pinned by the
hand-computed cases of ``tests/test_box_ap_cpu.py`` -- and runs it on the device:

  * ``stlpose::box_ap_match`` (evaluateImg: per (image, category) sort, fp64 IoU, greedy match for 10 thresholds x 4 area ranges),
  * one global stable score order per category (two ``torch.sort(stable=True)`` over all slots: by score, then by category),
  * ``stlpose::box_ap_accumulate`` (accumulate: prefix counts, recall, the 101-point precision envelope),

and the 12 means of ``summarize`` on the host.  Scores are float32, as a detector returns them; the ground truth and the boxes
are float64.  Caps: ``capi.BOX_MAX`` detections per image, ``capi.BOX_AP_GT_MAX`` ground truths per (image, category).
Keypoint AP is ``keypoint_eval.keypoint_ap`` (on the device, through the same accumulate kernel) or ``evaluate.oks_ap`` (host).
"""
from __future__ import annotations

import json
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import capi
from .detections import Detections, DetectionStore
from .coco_tables import REC_THRS, device_of, match_and_accumulate, mean_valid as mean, offsets_of, segment_rows, take_images

IOU_THRS = np.linspace(.5, 0.95, 10)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))   # all, small, medium, large
STAT_NAMES = ("AP", "AP50", "AP75", "AP(S)", "AP(M)", "AP(L)", "AR@1", "AR@10", "AR@100", "AR(S)", "AR(M)", "AR(L)")


class GroundTruth:
    """COCO box annotations as a ragged device table, images ascending by id: uploaded once, sliced per evaluation."""

    def __init__(self, annotations: Sequence[dict], cat_ids: Optional[Iterable[int]] = None, device=None):
        anns = sorted(annotations, key=lambda a: a["image_id"])   # stable: annotation order within an image
        ids = np.asarray([a["image_id"] for a in anns], np.int64)
        self.img_ids, self.counts = np.unique(ids, return_counts=True)
        self.labels_host = np.asarray([a["category_id"] for a in anns], np.int64)
        self.cat_ids = sorted(set(int(c) for c in cat_ids)) if cat_ids is not None else None
        self.device = device_of(device)
        box = np.asarray([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
        self.boxes = torch.from_numpy(box).to(self.device)
        self.area = torch.from_numpy(np.asarray([a["area"] for a in anns], np.float64)).to(self.device)
        self.labels = torch.from_numpy(self.labels_host).to(self.device)
        self.crowd = torch.from_numpy(np.asarray([bool(a.get("iscrowd", 0)) for a in anns], np.uint8)).to(self.device)

    def select(self, img_ids: np.ndarray):
        """The rows of the given images (ascending ids; an image without annotations has none): tensors and offsets.  For every
        image of the table, in order, these are the stored tables themselves, not copies."""
        (boxes, area, labels, crowd, labels_host), offsets = take_images(
            (self.boxes, self.area, self.labels, self.crowd, self.labels_host), self.img_ids, self.counts, img_ids, self.device)
        return boxes, area, labels, crowd, offsets, labels_host


class BoxEval:
    """What ``COCOeval`` holds after accumulate / summarize: ``precision`` [T, R, K, A, M], ``recall`` [T, K, A, M] (numpy,
    -1 where a category has no ground truth in an area range), ``stats`` [12], and ``params`` (the ids and thresholds used)."""

    def __init__(self):
        self.precision = self.recall = self.stats = None
        self.eval: dict = {}
        self.params: dict = {}


def evaluate_tables(boxes, scores, labels, det_offsets, gt: tuple, cat_ids: Sequence[int], max_dets=(1, 10, 100), img_ids=None):
    """match + order + accumulate on the device for ragged tables whose images are in ascending id order.  boxes float64 [N, 4]
    xywh, scores float32 [N], labels int64 [N], det_offsets int64 [I + 1] (CPU); gt = (boxes, area, labels, crowd, offsets).
    Returns (precision, recall) as device tensors.  img_ids (the tables' image ids, in table order): an exceeded cap is reported
    with the image's id instead of its position alone."""
    gb, ga, gl, gc, goff = gt
    cats = torch.tensor([int(c) for c in cat_ids], dtype=torch.int64)
    return match_and_accumulate(lambda: torch.ops.stlpose.box_ap_match(
        boxes, scores, labels, det_offsets, gb, ga, gl, gc, goff, cats, [float(t) for t in IOU_THRS],
        [float(v) for r in AREA_RANGES for v in r]), cats.shape[0], len(IOU_THRS), max_dets, img_ids)


def summarize(precision: np.ndarray, recall: np.ndarray) -> np.ndarray:
    """COCOeval.summarize for "bbox": the 12 numbers of ``STAT_NAMES``, each the mean of the entries > -1, or -1.  AP and the
    per-area numbers are read at the last maxDets, AR at each of the three."""
    t50, t75 = 0, 5
    last = precision.shape[4] - 1
    return np.array([mean(precision[:, :, :, 0, last]), mean(precision[t50, :, :, 0, last]), mean(precision[t75, :, :, 0, last]),
                     mean(precision[:, :, :, 1, last]), mean(precision[:, :, :, 2, last]), mean(precision[:, :, :, 3, last]),
                     mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
                     mean(recall[:, :, 1, last]), mean(recall[:, :, 2, last]), mean(recall[:, :, 3, last])])


def _check_max_dets(max_dets):
    md = [int(m) for m in max_dets]
    if len(md) != 3 or md != sorted(md) or md[0] < 1 or md[-1] > capi.BOX_AP_DETS:
        raise ValueError(f"box AP: max_dets must be three rising values in 1 .. {capi.BOX_AP_DETS} (STL_BOX_AP_DETS), got {max_dets}")
    return md


def box_ap(gt_annotations: Sequence[dict], results: Sequence[dict], img_ids: Optional[Sequence[int]] = None,
           max_dets: Sequence[int] = (1, 10, 100), cat_ids: Optional[Sequence[int]] = None, device=None) -> np.ndarray:
    """Box AP/AR with COCOeval semantics, the counterpart of ``oks_ap``.  gt_annotations: COCO annotation dicts (image_id, category_id,
    bbox xywh, area, iscrowd); results: COCO result dicts (image_id, category_id, bbox xywh, score).  img_ids: the images to score
    (default: every image either list names); cat_ids: the categories (default: every category either list names; one without
    ground truth yields -1 entries, which no mean counts).  Returns the 12 numbers of COCOeval.stats for bbox: AP, AP50, AP75,
    AP(S), AP(M), AP(L), AR@1, AR@10, AR@100, AR(S), AR(M), AR(L)."""
    md = _check_max_dets(max_dets)
    dev = device_of(device)
    if img_ids is None:
        img_ids = {a["image_id"] for a in gt_annotations} | {r["image_id"] for r in results}
    if cat_ids is None:
        cat_ids = {a["category_id"] for a in gt_annotations} | {r["category_id"] for r in results}
    ids = np.asarray(sorted(set(int(i) for i in img_ids)), np.int64)
    cats = sorted(set(int(c) for c in cat_ids))
    table = GroundTruth(gt_annotations, device=dev)
    res = sorted((r for r in results), key=lambda r: r["image_id"])   # stable: result order within an image
    rid = np.asarray([r["image_id"] for r in res], np.int64)
    keep = np.isin(rid, ids)
    cnt = np.bincount(np.searchsorted(ids, rid[keep]), minlength=len(ids)).astype(np.int64)
    res = [r for r, k in zip(res, keep) if k]
    boxes = torch.from_numpy(np.asarray([r["bbox"] for r in res], np.float64).reshape(-1, 4)).to(dev)
    scores = torch.from_numpy(np.asarray([r["score"] for r in res], np.float32)).to(dev)
    labels = torch.from_numpy(np.asarray([r["category_id"] for r in res], np.int64)).to(dev)
    offsets = torch.from_numpy(offsets_of(cnt))
    precision, recall = evaluate_tables(boxes, scores, labels, offsets, table.select(ids)[:5], cats, md, img_ids=ids)
    return summarize(precision.cpu().numpy(), recall.cpu().numpy())


def _annotations_of(coco_gt):
    """(annotation dicts, category ids or None) of a list, a path to a COCO json, or an object with .dataset."""
    if isinstance(coco_gt, str):
        with open(coco_gt) as f:
            coco_gt = json.load(f)
    ds = coco_gt if isinstance(coco_gt, dict) else getattr(coco_gt, "dataset", None)
    if ds is not None:
        cats = [c["id"] for c in ds["categories"]] if ds.get("categories") else None
        return ds["annotations"], cats
    return list(coco_gt), None


class CocoEvaluator:
    """The reference's ``CocoEvaluator`` for ``iou_types=("bbox",)`` with its methods, so that its validation loops port by changing
    the import.  coco_gt: a list of annotation dicts, a path to a COCO json, or any object with ``.dataset["annotations"]`` (a
    pycocotools ``COCO``); it is uploaded once, here.  The categories are the dataset's ``categories`` where it has them, else every
    category the annotations or the predictions name."""

    def __init__(self, coco_gt, iou_types=("bbox",), device=None, store_capacity: int = 1 << 20):
        iou_types = [iou_types] if isinstance(iou_types, str) else list(iou_types)
        for t in iou_types:
            if t != "bbox":
                raise NotImplementedError(f"CocoEvaluator: iou_type {t!r}; box AP only ('bbox').  Keypoint AP is "
                                          "stlpose_amd.evaluate.oks_ap; 'segm' is not provided")
        self.iou_types = iou_types
        self.device = device_of(device)
        # a GroundTruth built earlier is taken as it is: a training loop that validates every epoch uploads it once
        self.gt = coco_gt if isinstance(coco_gt, GroundTruth) else GroundTruth(*_annotations_of(coco_gt), device=self.device)
        self.coco_eval: Dict[str, BoxEval] = {"bbox": BoxEval()}
        self.img_ids: List[int] = []
        self._chunks: list = []    # per update: (image ids, rows per image, boxes xywh f64, scores f32, labels i64) on the device
        self._tables = None
        self.store_capacity = int(store_capacity)   # rows of the DetectionStore that update(image_ids, Detections) fills
        self._store: Optional[DetectionStore] = None

    # -- collecting
    def update(self, predictions, detections: Optional[Detections] = None) -> None:
        """predictions: {image_id: {"boxes" [n, 4] xyxy, "labels" [n], "scores" [n]}}, CPU or device tensors.  The boxes become xywh
        as the reference's convert_to_xywh makes them (the subtraction in the tensor's own dtype) and stay on the device; nothing
        here waits for the device.  ``update(image_ids, detections)`` takes a batch as ``Detections`` (forward(output="device"))
        with one id per image: one launch into a ``DetectionStore`` of ``store_capacity`` rows."""
        if detections is not None or isinstance(predictions, Detections):
            if not isinstance(detections, Detections):
                raise TypeError("CocoEvaluator.update: (image_ids, Detections) or {image_id: prediction}")
            if self._store is None:
                self._store = DetectionStore(self.store_capacity, self.device)
            ids = [int(i) for i in predictions]
            self._store.append(ids, detections)
            self.img_ids.extend(sorted(set(ids)))
            self._tables = None
            return
        ids, cnt, bs, ss, ls = [], [], [], [], []
        for image_id, p in predictions.items():
            b = torch.as_tensor(p["boxes"]).reshape(-1, 4)
            s = torch.as_tensor(p["scores"]).reshape(-1)
            l = torch.as_tensor(p["labels"]).reshape(-1)
            if not (b.shape[0] == s.shape[0] == l.shape[0]):
                raise ValueError(f"CocoEvaluator.update: image {image_id}: {b.shape[0]} boxes, {s.shape[0]} scores, {l.shape[0]} labels")
            ids.append(int(image_id)), cnt.append(b.shape[0]), bs.append(b), ss.append(s), ls.append(l)
        if not ids:
            return
        def gather(ts):   # one copy per update when the tensors share a device (the reference hands over CPU tensors)
            if len({t.device for t in ts}) == 1:
                return torch.cat(ts).to(self.device, non_blocking=True)
            return torch.cat([t.to(self.device, non_blocking=True) for t in ts])
        b = gather(bs)
        xywh = torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], 1).double()
        s, l = gather(ss).float(), gather(ls).long()
        self.img_ids.extend(sorted(set(ids)))
        self._chunks.append((np.asarray(ids, np.int64), np.asarray(cnt, np.int64), xywh, s, l))
        self._tables = None

    def synchronize_between_processes(self, process_group=None) -> None:
        """Builds the evaluation tables: the updates concatenated (with a process group: all-gathered first, ranks in order),
        each image id once -- its first occurrence, as ``np.unique`` picks it in the reference's merge -- and ascending."""
        chunks = list(self._chunks)   # the dict updates in order, then the store's batches in order
        if self._store is not None and self._store.num_slots:
            chunks.append(self._store.finish())
        if chunks:
            ids = np.concatenate([c[0] for c in chunks])
            cnt = np.concatenate([c[1] for c in chunks])
            boxes, scores, labels = (torch.cat([c[i] for c in chunks]) if len(chunks) > 1 else chunks[0][i] for i in (2, 3, 4))
        else:
            ids, cnt = np.zeros(0, np.int64), np.zeros(0, np.int64)
            boxes = torch.zeros(0, 4, dtype=torch.float64, device=self.device)
            scores = torch.zeros(0, dtype=torch.float32, device=self.device)
            labels = torch.zeros(0, dtype=torch.int64, device=self.device)
        if process_group is not None:
            import torch.distributed as dist
            parts = [None] * dist.get_world_size(process_group)
            dist.all_gather_object(parts, (ids, cnt, boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()), group=process_group)
            ids, cnt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            boxes, scores, labels = (torch.from_numpy(np.concatenate([p[i] for p in parts])).to(self.device) for i in (2, 3, 4))
        uniq, first = np.unique(ids, return_index=True)     # ascending ids, first occurrence of each
        start = (np.cumsum(cnt) - cnt)[first]
        rows = torch.from_numpy(segment_rows(start, cnt[first])).to(self.device)
        offsets = torch.from_numpy(offsets_of(cnt[first]))
        self._tables = (uniq, boxes[rows], scores[rows], labels[rows], offsets)
        self.img_ids = [int(i) for i in uniq]

    # -- scoring
    def accumulate(self, max_dets: Sequence[int] = (1, 10, 100)) -> None:
        if self._tables is None:
            self.synchronize_between_processes()
        md = _check_max_dets(max_dets)
        uniq, boxes, scores, labels, offsets = self._tables
        sel = self.gt.select(uniq)
        cats = self.gt.cat_ids
        if cats is None:   # no category list in the dataset: every category named by the scored images' ground truth or detections
            cats = sorted(set(sel[5].tolist()) | set(torch.unique(labels).cpu().tolist()))
        ev = self.coco_eval["bbox"]
        precision, recall = evaluate_tables(boxes, scores, labels, offsets, sel[:5], cats, md, img_ids=uniq)
        ev.precision, ev.recall = precision.cpu().numpy(), recall.cpu().numpy()
        ev.params = dict(imgIds=[int(i) for i in uniq], catIds=list(cats), iouThrs=IOU_THRS, recThrs=REC_THRS, maxDets=md,
                         areaRng=[list(r) for r in AREA_RANGES], areaRngLbl=["all", "small", "medium", "large"])
        ev.eval = dict(params=ev.params, counts=[len(IOU_THRS), len(REC_THRS), len(cats), len(AREA_RANGES), len(md)],
                       precision=ev.precision, recall=ev.recall)

    def summarize(self) -> Dict[str, np.ndarray]:
        ev = self.coco_eval["bbox"]
        if ev.precision is None:
            self.accumulate()
        ev.stats = summarize(ev.precision, ev.recall)
        md = ev.params["maxDets"]
        rows = [(1, "0.50:0.95", "all", md[2]), (1, "0.50", "all", md[2]), (1, "0.75", "all", md[2]), (1, "0.50:0.95", "small", md[2]),
                (1, "0.50:0.95", "medium", md[2]), (1, "0.50:0.95", "large", md[2]), (0, "0.50:0.95", "all", md[0]),
                (0, "0.50:0.95", "all", md[1]), (0, "0.50:0.95", "all", md[2]), (0, "0.50:0.95", "small", md[2]),
                (0, "0.50:0.95", "medium", md[2]), (0, "0.50:0.95", "large", md[2])]
        print("IoU metric: bbox")
        for (ap, iou, area, m), v in zip(rows, ev.stats):
            title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
            print(f" {title:<18} {kind} @[ IoU={iou:<9} | area={area:>6s} | maxDets={m:>3d} ] = {v:0.3f}")
        return {"bbox": ev.stats}


def _is_det_batch(imgs) -> bool:
    from .det_data import DetBatch
    return isinstance(imgs, DetBatch)


class DetectorEvaluator:
    """The evaluation loop of ``03_evaluate_faster_rcnn.py:133-167`` (and, with ``fraction=0.2``, the validation epoch of
    ``02_train_faster_rcnn.py:241-280``, which scores the first fifth of the loader).  The loader yields ``(imgs, metas)``: images
    with values in 0 .. 255 (a stacked tensor or a list of CHW tensors), or a ``det_data.DetBatch`` (``DetBatchLoader``), which goes to
    the model as it is, and one dict per image with ``image_id``.  With a
    process group, rank r runs batches r, r + world, ... and every rank scores the gathered set.  An indexable loader (a list
    of batches, a map-style dataset of batches: ``__len__`` and ``__getitem__``) is indexed directly, so a rank never loads the
    batches of the others; a plain iterable can only be skipped through, which loads them all."""

    def __init__(self, model, process_group=None, device=None, output="host"):
        """output="device": the model's detections stay on the device (``forward(output="device")``) and are collected with one
        launch per batch; the scores are the same."""
        if output not in ("host", "device"):
            raise ValueError(f"DetectorEvaluator: output {output!r} (one of 'host', 'device')")
        self.model, self.pg, self.device, self.output = model, process_group, device_of(device), output
        self.rank, self.world = 0, 1
        if process_group is not None:
            import torch.distributed as dist
            self.rank, self.world = dist.get_rank(process_group), dist.get_world_size(process_group)
        self.coco_evaluator: Optional[CocoEvaluator] = None

    def _my_batches(self, loader, limit):
        """The batches this rank runs: r, r + world, ... below ``limit`` (None: all), as ``Evaluator._my_batches`` shards them."""
        if self.world > 1 and hasattr(loader, "__getitem__") and hasattr(loader, "__len__"):
            for i in range(self.rank, len(loader) if limit is None else min(limit, len(loader)), self.world):
                yield loader[i]
            return
        for i, batch in enumerate(loader):
            if limit is not None and i >= limit:
                break
            if i % self.world == self.rank:
                yield batch

    @torch.no_grad()
    def evaluate(self, loader: Iterable, coco_gt, fraction: float = 1.0) -> dict:
        if not 0.0 < fraction <= 1.0:
            raise ValueError(f"DetectorEvaluator: fraction {fraction} (0 < fraction <= 1)")
        self.model.eval()
        ev = self.coco_evaluator = CocoEvaluator(coco_gt, ("bbox",), device=self.device)
        limit = None if fraction == 1.0 else int(np.floor(len(loader) * fraction + 1e-9))
        for imgs, metas in self._my_batches(loader, limit):
            if _is_det_batch(imgs):   # det_data.DetBatchLoader: the batch is the network's input already, on the device
                out = self.model(imgs, output=self.output)
                if self.output == "device":
                    ev.update([int(meta["image_id"]) for meta in metas], out)
                else:
                    ev.update({int(meta["image_id"]): o for meta, o in zip(metas, out)})
                continue
            if isinstance(imgs, (list, tuple)):
                imgs = torch.stack(list(imgs))
            if self.output == "device":
                ev.update([int(meta["image_id"]) for meta in metas], self.model(imgs.to(self.device).float() / 255, output="device"))
                continue
            outputs = self.model(imgs.to(self.device).float() / 255)
            ev.update({int(meta["image_id"]): out for meta, out in zip(metas, outputs)})
        ev.synchronize_between_processes(self.pg)
        ev.accumulate()
        stats = ev.summarize()["bbox"]
        return {"stats": stats, "valid_ap": float(stats[0])}
