"""The detector's outputs as device tables: one batch (``Detections``) and an epoch's ragged store (``DetectionStore``).

``EfficientDetBackbone.forward(..., output="device")`` ends in one launch of ``stlpose::det_postprocess`` (decode, sort, class-aware
NMS and the inverse resize, ``csrc/detections.hip``) and returns a ``Detections``; nothing waits for the device until somebody asks
for host values.  ``Detections.to_list()`` is that request for one batch: one copy, then exactly the list ``forward`` returns by
default.  ``DetectionStore`` collects batches with one launch each (``stlpose::det_append``) and copies its slot table once, in
``finish()``; ``CocoEvaluator.update(image_ids, detections)`` feeds one.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import capi

SLOTS0 = 1024   # image slots a store starts with; the slot table doubles when it is full (a device copy, no wait)


class Detections:
    """One batch of final detections: ``boxes`` float32 [B, K, 4] (x1, y1, x2, y2), ``scores`` float32 [B, K], ``labels`` int32
    [B, K] (class + 1) and ``count`` int32 [B], K = ``capi.BOX_MAX``; image i owns rows 0 .. count[i] - 1, in keep order.  A count of
    -n - 1 marks an image whose n candidates exceeded K: it has no rows."""

    def __init__(self, boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, count: torch.Tensor):
        b = count.shape[0]
        if count.dim() != 1 or boxes.dim() != 3 or boxes.shape[0] != b or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) \
                or tuple(labels.shape) != tuple(boxes.shape[:2]):
            raise ValueError(f"Detections: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, labels {tuple(labels.shape)}, count "
                             f"{tuple(count.shape)} are not [B, K, 4], [B, K], [B, K], [B]")
        self.boxes, self.scores, self.labels, self.count = boxes, scores, labels, count

    def __len__(self) -> int:
        return self.count.shape[0]

    @property
    def device(self) -> torch.device:
        return self.count.device

    def host_tables(self):
        """(boxes, scores, labels, count) as numpy arrays: for device tables one packed copy, the call's only wait."""
        if self.count.device.type == "cpu":
            return self.boxes.numpy(), self.scores.numpy(), self.labels.numpy(), self.count.numpy()
        b, k = self.scores.shape
        parts = (self.count.to(torch.int32), self.boxes.float(), self.scores.float(), self.labels.to(torch.int32))
        blob = torch.cat([p.contiguous().view(-1).view(torch.uint8) for p in parts]).cpu().numpy()
        cut = np.cumsum([0, b * 4, b * k * 16, b * k * 4, b * k * 4])
        count, boxes, scores, labels = (blob[cut[i]:cut[i + 1]] for i in range(4))
        return (boxes.view(np.float32).reshape(b, k, 4), scores.view(np.float32).reshape(b, k), labels.view(np.int32).reshape(b, k),
                count.view(np.int32))

    def to_list(self) -> List[Dict[str, torch.Tensor]]:
        """What ``EfficientDetBackbone.forward`` returns with output="host": per image {"boxes" float32 [k, 4], "labels" int32 [k],
        "scores" float32 [k]} as CPU tensors (an image without detections: three empty 1-D tensors).  ValueError for an image
        above the candidate cap."""
        boxes, scores, labels, count = self.host_tables()
        out = []
        for i, n in enumerate(count.tolist()):
            if n < 0:
                raise ValueError(f"Detections: image {i} of the batch has {-n - 1} candidates above the threshold; the device path holds "
                                 f"at most {capi.BOX_MAX} (STL_BOX_MAX) per image.  Raise the threshold or use output='host'")
            if n == 0:
                out.append({"boxes": torch.zeros(0), "labels": torch.zeros(0, dtype=torch.int32), "scores": torch.zeros(0)})
                continue
            out.append({"boxes": torch.from_numpy(boxes[i, :n].copy()), "labels": torch.from_numpy(labels[i, :n].copy()),
                        "scores": torch.from_numpy(scores[i, :n].copy())})
        return out


class DetectionStore:
    """A ragged store of detections on ``device``: ``boxes`` float64 [capacity_rows, 4] xywh (as the reference's convert_to_xywh
    makes them: subtracted in float32, then widened), ``scores`` float32, ``labels`` int64, and per appended image a slot
    (image id, first row, count).  Rows are laid out in append order, images in batch order, so the tables are deterministic."""

    def __init__(self, capacity_rows: int, device):
        if int(capacity_rows) < 0:
            raise ValueError(f"DetectionStore: capacity_rows {capacity_rows}")
        self.capacity, self.device = int(capacity_rows), torch.device(device)
        self.boxes = torch.empty(self.capacity, 4, dtype=torch.float64, device=self.device)
        self.scores = torch.empty(self.capacity, dtype=torch.float32, device=self.device)
        self.labels = torch.empty(self.capacity, dtype=torch.int64, device=self.device)
        # row 0: (cursor of even appends, cursor of odd appends, overflow flag); rows 1 ..: the slots.  One table, one copy.
        self.table = torch.zeros(1 + SLOTS0, 3, dtype=torch.int64, device=self.device)
        self.num_slots = self.appends = 0

    def append(self, image_ids: Sequence[int], detections: Detections) -> None:
        """One launch; never waits for the device.  image_ids: one id per image of the batch."""
        ids = [int(i) for i in image_ids]
        if len(ids) != len(detections):
            raise ValueError(f"DetectionStore.append: {len(ids)} image ids for a batch of {len(detections)}")
        if not ids:
            return
        while self.num_slots + len(ids) > self.table.shape[0] - 1:
            self.table = torch.cat([self.table, torch.zeros(self.table.shape[0] - 1, 3, dtype=torch.int64, device=self.device)])
        idt = torch.tensor(ids, dtype=torch.int64).to(self.device, non_blocking=True)
        d = detections
        torch.ops.stlpose.det_append(d.boxes, d.scores, d.labels, d.count, idt, self.boxes, self.scores, self.labels, self.table[1:],
                                     self.num_slots, self.table[0, :2], self.appends & 1, self.table[0, 2:])
        self.num_slots += len(ids)
        self.appends += 1

    def finish(self):
        """The epoch's one copy (the slot table).  Returns (image ids int64 [I], counts int64 [I]) as numpy arrays in append order
        and (boxes float64 [N, 4] xywh, scores float32 [N], labels int64 [N]) on the device, N = the counts' sum: the form
        ``CocoEvaluator.synchronize_between_processes`` concatenates its updates into."""
        return self.tables_of(self.table[:1 + self.num_slots].cpu().numpy(), self.appends)

    def tables_of(self, table: np.ndarray, appends: int):
        """finish() from the host copy of the slot table."""
        ids, start, cnt = (table[1:, i] for i in range(3))
        if table[0, 2] != 0:
            raise ValueError(f"DetectionStore: the store's capacity of {self.capacity} rows was exceeded "
                             f"({int(np.maximum(cnt, 0).sum())} rows appended); build it with a larger capacity_rows")
        if (cnt < 0).any():
            i = int(np.argmax(cnt < 0))
            raise ValueError(f"DetectionStore: image id {int(ids[i])} has {int(-cnt[i] - 1)} candidates above the threshold; the device "
                             f"path holds at most {capi.BOX_MAX} (STL_BOX_MAX) per image")
        total = int(table[0, appends & 1])
        assert total == int(cnt.sum()) and (len(cnt) == 0 or np.array_equal(start, np.cumsum(cnt) - cnt))
        return ids.copy(), cnt.copy(), self.boxes[:total], self.scores[:total], self.labels[:total]
