"""Detector training / validation batches built on the GPU from COCO box annotations (reference ``data/Detection_Dataset.py`` +
``ResizeImageDetection`` of ``data/custom_transforms.py:36-67`` + ``get_detection_dataset`` and the ``DataLoader`` of
``data/data_loaders.py``), the detector's counterpart of ``pose_data``.

Three parts:

  * ``coco_detection_db``: a COCO instances file -> one table row per kept image and one per kept box
    (``Detection_Dataset.py:128-213``), host numpy.  pycocotools is not a dependency: the JSON is read directly, so the reading order
    and the filters are this module's reading of ``pycocotools.coco.COCO`` (images in file order, an image's annotations in file
    order, ``getAnnIds(iscrowd=False)`` leaves the crowd annotations out, ``getCatIds()`` is the file's category order).  **Parity with
    pycocotools is unpinned**: nothing here was compared with it; ``tests/test_det_batch_cpu.py`` pins the rules by hand-computed
    cases.
  * ``pose_data.ResidentImages`` / ``StreamedImages`` hold the decoded uint8 images, unchanged.
  * ``DetBatchLoader``: ONE launch per batch (``stlpose::det_batch``, csrc/det_batch.hip) that fills the network's canvas and the
    ground-truth table ``stl_det_loss`` reads, and no per-image Python arithmetic.  With ``ResidentImages`` the host never waits for
    the device between the first and the last batch of an epoch.  The resize follows this library's statement of
    ``cv2.resize(INTER_LINEAR)`` in fp32; cv2 blends uint8 images in 11-bit fixed point and can differ by one level: **unpinned**
    (include/stlpose_hip_det_batch.h).

``EfficientDetBackbone.forward`` / ``detection_loss`` and ``DetectorEvaluator`` take the loader's ``DetBatch`` as it is.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)
from .efficientdet import MAX_SIZE, resize_meta
from .pose_data import epoch_indices


# ---------------------------------------------------------------------------------------------------------------- tables
def resized_size(height: int, width: int, image_size: int) -> Tuple[float, int, int]:
    """ResizeImageDetection.__call__'s (scale, resized_height, resized_width), in Python floats as there."""
    if height > width:
        scale = image_size / height
        return scale, image_size, int(width * scale)
    scale = image_size / width
    return scale, int(height * scale), image_size


@dataclass
class DetectionDB:
    """One row per kept image, one per kept box; image k owns rows ``box_start[k] : box_start[k] + box_count[k]`` of the box tables."""
    image_id: np.ndarray           # (K,) int64
    file_name: List[str]           # the (styled) image's file name
    original_name: List[str]       # '%012d.jpg' % image_id
    height: np.ndarray             # (K,) int32
    width: np.ndarray              # (K,) int32
    perceptual_loss: np.ndarray    # (K,) float64, 0 without a dictionary
    box_start: np.ndarray          # (K,) int64
    box_count: np.ndarray          # (K,) int32
    boxes: np.ndarray              # (N, 4) float32 x1, y1, x2, y2 in source pixels (clean_bbox)
    labels: np.ndarray             # (N,) int64 class index, 1 = the file's first category
    area: np.ndarray               # (N,) float64, the file's value
    class_ids: Tuple[int, ...] = (1,)
    _device_tables: dict = field(default_factory=dict, repr=False)

    def __len__(self) -> int:
        return int(self.image_id.shape[0])

    def image_sizes(self) -> List[Tuple[int, int]]:
        """(height, width) of every image, for ``ResidentImages.from_files``."""
        return [(int(h), int(w)) for h, w in zip(self.height, self.width)]

    def scales(self, image_size: int) -> np.ndarray:
        """The resizer's ``scale`` of every image, float64 [K]."""
        return np.asarray([resized_size(int(h), int(w), image_size)[0] for h, w in zip(self.height, self.width)], np.float64).reshape(-1)

    def scaled_boxes(self, image_size: int) -> np.ndarray:
        """``annots["boxes"] *= scale`` (custom_transforms.py:63) on the float32 boxes: the product in float32, [N, 4]."""
        per_box = np.repeat(self.scales(image_size).astype(np.float32), self.box_count)
        return (self.boxes * per_box[:, None]).astype(np.float32)

    def coco_gt(self, image_size: int) -> dict:
        """What ``get_coco_api_from_dataset`` (lib/detection_coco_utils.py:146-196) hands the evaluator for this table behind
        ``ResizeImageDetection(image_size)``, as a dict ``CocoEvaluator`` / ``GroundTruth`` accept: the boxes scaled in float32 and
        made xywh by the float32 subtraction, ``area`` the file's unscaled value (as the reference has it), ``iscrowd`` 0, annotation
        ids from 1, the categories the sorted labels that occur."""
        b = self.scaled_boxes(image_size)
        b[:, 2:] -= b[:, :2]
        owner = np.repeat(self.image_id, self.box_count)
        anns = [{"image_id": int(owner[i]), "bbox": [float(v) for v in b[i]], "category_id": int(self.labels[i]),
                 "area": float(self.area[i]), "iscrowd": 0, "id": i + 1} for i in range(b.shape[0])]
        images = [{"id": int(i), "height": int(image_size), "width": int(image_size)} for i in self.image_id]
        return {"images": images, "categories": [{"id": int(c)} for c in sorted(set(self.labels.tolist()))], "annotations": anns}

    def device_tables(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(box_start, box_count, boxes, labels) on ``device``, uploaded once."""
        dev = torch.device(device)
        if dev not in self._device_tables:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
            self._device_tables[dev] = (up(self.box_start), up(self.box_count), up(self.boxes), up(self.labels))
        return self._device_tables[dev]


def coco_detection_db(annotations, class_ids: Sequence[int] = (1,), mapping: Optional[Dict[str, str]] = None,
                      perceptual_loss: Optional[Dict[str, float]] = None) -> DetectionDB:
    """``annotations``: the parsed COCO instances JSON (a dict with "images", "annotations" and "categories") or its path.
    ``class_ids``: the class indices kept (1 + a category's position among the file's categories; default the first, person).
    ``mapping``: the Styled-COCO dictionary '%012d' % image_id -> styled file name (``_image_name_from_index``; a missing id is a
    KeyError, as there).  ``perceptual_loss``: file name -> precomputed loss (Detection_Dataset.py:104-106)."""
    if isinstance(annotations, (str, os.PathLike)):
        with open(annotations) as f:
            annotations = json.load(f)
    class_of = {c["id"]: 1 + k for k, c in enumerate(annotations.get("categories", []))}   # _coco_ind_to_class_ind
    keep = {int(c) for c in class_ids}
    by_image: Dict[int, list] = {}
    for ann in annotations["annotations"]:
        by_image.setdefault(ann["image_id"], []).append(ann)
    ids, names, originals, hs, ws, perc, starts, counts = [], [], [], [], [], [], [], []
    boxes, labels, areas = [], [], []
    for im in annotations["images"]:
        width, height = im["width"], im["height"]
        n0 = len(boxes)
        for obj in by_image.get(im["id"], []):
            if obj.get("iscrowd", 0):
                continue
            x, y, w, h = obj["bbox"]
            x1, y1 = max(0, x), max(0, y)                                    # :176-185
            x2 = min(width - 1, x1 + max(0, w - 1))
            y2 = min(height - 1, y1 + max(0, h - 1))
            if not (obj["area"] > 0 and x2 >= x1 and y2 >= y1):
                continue
            cls = class_of[obj["category_id"]]
            if cls not in keep:
                continue
            boxes.append([x1, y1, x2, y2]), labels.append(cls), areas.append(obj["area"])
        if len(boxes) == n0:   # :142: an image without a box is skipped
            continue
        original = "%012d.jpg" % im["id"]
        name = mapping[original[:-4]] if mapping is not None else original
        ids.append(int(im["id"])), names.append(name), originals.append(original), hs.append(int(height)), ws.append(int(width))
        perc.append(float(perceptual_loss[name]) if perceptual_loss else 0.0)
        starts.append(n0), counts.append(len(boxes) - n0)
    return DetectionDB(image_id=np.asarray(ids, np.int64).reshape(-1), file_name=names, original_name=originals,
                       height=np.asarray(hs, np.int32).reshape(-1), width=np.asarray(ws, np.int32).reshape(-1),
                       perceptual_loss=np.asarray(perc, np.float64).reshape(-1), box_start=np.asarray(starts, np.int64).reshape(-1),
                       box_count=np.asarray(counts, np.int32).reshape(-1), boxes=np.asarray(boxes, np.float32).reshape(-1, 4),
                       labels=np.asarray(labels, np.int64).reshape(-1), area=np.asarray(areas, np.float64).reshape(-1),
                       class_ids=tuple(sorted(keep)))


# ---------------------------------------------------------------------------------------------------------------- the batch
@dataclass
class DetBatch:
    """One batch on the device, as ``EfficientDetBackbone`` takes it: ``canvas`` fp32 NHWC [B, S, S, 3] (the network's input, after
    ResizeImageDetection, / 255, Normalize and the resize to the canvas), ``gt`` fp32 [rows, 5] and ``offsets`` int32 [B + 1] (the
    table ``stl_det_loss`` reads), ``image_size`` = S1 and ``meta`` = ``resize_meta(S1, S1)``: detections come back on the S1 x S1
    image's scale, which is where ``DetectionDB.coco_gt(S1)`` has the ground truth."""
    canvas: torch.Tensor
    gt: torch.Tensor
    offsets: torch.Tensor
    image_size: int
    meta: tuple
    perceptual_loss: Optional[torch.Tensor] = None   # CPU float64 [B]
    stage1: Optional[torch.Tensor] = None            # uint8 [B, S1, S1, 3], on request

    def __len__(self) -> int:
        return int(self.canvas.shape[0])


def det_batch(images_rows, index: torch.Tensor, tables, draws: Optional[torch.Tensor], flip: bool, image_size: int, gt_rows: int,
              canvas_size: int = MAX_SIZE, stage1: bool = False, canvas: Optional[torch.Tensor] = None) -> DetBatch:
    """One launch of ``stlpose::det_batch``.  images_rows: ``ResidentImages.rows(...)`` of the chosen images; index int64 [B]: their
    rows in ``tables`` = ``DetectionDB.device_tables``; gt_rows: the batch's box count (known from the host table)."""
    src, off, hw = images_rows
    b = int(index.shape[0])
    if canvas is None:
        canvas = torch.empty(b, canvas_size, canvas_size, 3, dtype=torch.float32, device=src.device)
    s1, gt, offsets = torch.ops.stlpose.det_batch(canvas, src, off, hw, index, *tables, draws, bool(flip), int(image_size), int(gt_rows),
                                                  bool(stage1))
    return DetBatch(canvas, gt, offsets, int(image_size), resize_meta(int(image_size), int(image_size), int(canvas.shape[1])),
                    stage1=s1 if stage1 else None)


# ---------------------------------------------------------------------------------------------------------------- the loader
class DetBatchLoader:
    """An iterable of ``(batch, metas)``: a ``DetBatch`` and one dict per image with the reference's keys ``image_id``, ``image_name``,
    ``original_image_name``, ``scale``, ``original_size`` and ``perceptual_loss`` (Detection_Dataset.py:108-116; all from host tables,
    nothing is copied back) -- what ``DetectorTrainer`` and ``DetectorEvaluator`` consume.  ``image_size`` is ResizeImageDetection's
    (``exp_data["dataset"]["image_size"]`` when it is not given; 400 as there otherwise).

    Every ``iter()`` is a new epoch (``set_epoch`` chooses it): its permutation (``epoch_indices``) and the flip draws (a device
    generator seeded from ``(seed, epoch, rank)``) go up before the first batch, so the same ``(seed, epoch)`` gives the same batches
    bit for bit.  The training loader shuffles and drops the ragged last batch; the validation loader does neither and can be
    indexed (``len(loader)``, ``loader[i]``), so ``DetectorEvaluator`` shards it.  The horizontal flip is off unless
    ``exp_data["dataset"]["flip"]`` is true (the reference has none for detection) and applies to the training loader only.

    ``loader.last`` holds the kernel's inputs of the batch just made (``index``, ``draws``, the image rows), so it can be replayed.
    ``stage1=True`` also keeps the resized uint8 images in ``batch.stage1``."""

    def __init__(self, db: DetectionDB, images, exp_data: Optional[dict], batch_size: int, is_train: bool, image_size: Optional[int] = None,
                 seed: int = 0, rank: int = 0, world: int = 1, canvas_size: int = MAX_SIZE, stage1: bool = False, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("DetBatchLoader (HIP) needs a GPU device; there is no CPU path")
        if len(db) == 0:
            raise ValueError("DetBatchLoader: the image table is empty")
        if len(images) < len(db):
            raise ValueError(f"DetBatchLoader: the table has {len(db)} images, the store holds {len(images)}")
        if not 1 <= int(batch_size) <= capi.DET_BATCH_MAX:
            raise ValueError(f"DetBatchLoader: batch_size {batch_size} (1 .. {capi.DET_BATCH_MAX}, STL_DET_BATCH_MAX)")
        ds = (exp_data or {}).get("dataset", {})
        self.db, self.images, self.device = db, images, dev
        self.batch_size, self.is_train = int(batch_size), bool(is_train)
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.image_size = int(image_size if image_size is not None else ds.get("image_size", 400))
        self.canvas_size, self.stage1 = int(canvas_size), bool(stage1)
        self.flip = bool(ds.get("flip", False)) and self.is_train
        sizes = [resized_size(int(h), int(w), self.image_size) for h, w in zip(db.height, db.width)]
        if min(min(rh, rw) for _, rh, rw in sizes) < 1:
            raise ValueError(f"DetBatchLoader: an image resizes to an empty side at image_size {self.image_size}")
        self._scales = np.asarray([s for s, _, _ in sizes], np.float64)
        self._tables = db.device_tables(dev)
        self.meta = resize_meta(self.image_size, self.image_size, self.canvas_size)
        self.last: dict = {}

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _batches(self, epoch: int) -> List[np.ndarray]:
        return epoch_indices(len(self.db), self.batch_size, self.seed, epoch, self.rank, self.world, drop_last=self.is_train,
                             shuffle=self.is_train)

    def __len__(self) -> int:
        n, b = len(self.db), self.batch_size
        nb = n // b if self.is_train else -(-n // b)
        nb -= nb % self.world
        return len(range(self.rank, nb, self.world))

    def _draws(self, epoch: int, total: int) -> Optional[torch.Tensor]:
        if not self.flip:
            return None
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(np.random.SeedSequence([self.seed, epoch, self.rank]).generate_state(1, np.uint64)[0] >> np.uint64(1)))
        return torch.rand(total, dtype=torch.float64, device=self.device, generator=gen)

    def _make(self, rows: np.ndarray, index: torch.Tensor, draws: Optional[torch.Tensor], canvas: Optional[torch.Tensor] = None):
        """One batch: rows are the host's copy of index (the table rows of the chosen images)."""
        db = self.db
        with torch.cuda.device(self.device):
            image_rows = self.images.rows(index if self.images.device_resident else rows)
            batch = det_batch(image_rows, index, self._tables, draws, self.flip, self.image_size, int(db.box_count[rows].sum()),
                              self.canvas_size, self.stage1, canvas)
        batch.perceptual_loss = torch.from_numpy(db.perceptual_loss[rows])
        self.last = dict(index=index, draws=draws, rows=image_rows)
        metas = [{"image_id": int(db.image_id[k]), "image_name": db.file_name[k], "original_image_name": db.original_name[k],
                  "scale": float(self._scales[k]), "original_size": (int(db.height[k]), int(db.width[k])),
                  "perceptual_loss": float(db.perceptual_loss[k])} for k in rows]
        return batch, metas

    def __iter__(self):
        """Everything the epoch needs from the host goes up here, before the first batch: the indices and the draws."""
        epoch, self.epoch = self.epoch, self.epoch + 1
        batches = self._batches(epoch)
        total = int(sum(len(b) for b in batches))
        index = torch.from_numpy(np.concatenate(batches) if batches else np.zeros(0, np.int64)).to(self.device)
        return self._produce(batches, index, self._draws(epoch, total))

    def _produce(self, batches, index, draws):
        pos = 0
        for rows in batches:
            a, pos = pos, pos + len(rows)
            yield self._make(rows, index[a:pos], None if draws is None else draws[a:pos])

    def __getitem__(self, i: int):
        """Batch i of the validation order (the table's), on its own: what a rank of ``DetectorEvaluator`` asks for."""
        if self.is_train:
            raise TypeError("DetBatchLoader: a training loader is shuffled per epoch; iterate it")
        batches = self._batches(0)
        if not -len(batches) <= i < len(batches):
            raise IndexError(i)
        rows = batches[i]
        return self._make(rows, torch.from_numpy(rows).to(self.device), None)
