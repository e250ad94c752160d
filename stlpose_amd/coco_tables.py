"""What box AP (``detection_eval``) and keypoint AP (``keypoint_eval``) share on the host: ragged tables whose images ascend by
id, the step from a match op's slots to COCOeval's precision / recall, and the mean ``summarize`` takes."""
from __future__ import annotations

from typing import Callable, Sequence

import numpy as np
import torch

REC_THRS = np.linspace(.0, 1.0, 101)


def device_of(device) -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def offsets_of(cnt: np.ndarray) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


def segment_rows(start: np.ndarray, cnt: np.ndarray) -> np.ndarray:
    """concatenate(arange(start[i], start[i] + cnt[i]))"""
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(cnt) - cnt
    return np.repeat(start - first, cnt) + np.arange(total, dtype=np.int64)


def image_rows(table_ids: np.ndarray, counts: np.ndarray, starts: np.ndarray, img_ids: np.ndarray):
    """The rows of the images ``img_ids`` in a table whose image ``table_ids[i]`` (ascending) owns ``counts[i]`` rows from
    ``starts[i]``; an image the table does not name has none.  Returns (rows, offsets [len(img_ids) + 1])."""
    pos = np.searchsorted(table_ids, img_ids)
    has = pos < len(table_ids)
    has[has] = table_ids[pos[has]] == img_ids[has]
    cnt, start = np.zeros(len(img_ids), np.int64), np.zeros(len(img_ids), np.int64)
    cnt[has], start[has] = counts[pos[has]], starts[pos[has]]
    return segment_rows(start, cnt), offsets_of(cnt)


def take_images(tables: Sequence, table_ids: np.ndarray, counts: np.ndarray, img_ids, device):
    """``select`` of a ground-truth table stored image by image: the columns ``tables`` (device tensors or numpy arrays) cut down to
    the rows of ``img_ids`` (ascending), and their offsets as a CPU tensor."""
    img_ids = np.asarray(img_ids, np.int64)
    if np.array_equal(img_ids, table_ids):   # every image, in order: the tables as they are
        return list(tables), torch.from_numpy(offsets_of(counts))
    rows, offsets = image_rows(table_ids, counts, offsets_of(counts)[:-1], img_ids)
    r = torch.from_numpy(rows).to(device)
    return [t[r] if torch.is_tensor(t) else t[rows] for t in tables], torch.from_numpy(offsets)


def match_and_accumulate(match: Callable[[], tuple], num_cats: int, num_thrs: int, max_dets: Sequence[int], img_ids=None):
    """order + accumulate on the device behind a match op.  match() returns the op's slots (score, category, rank, matched,
    ignored, npig) for tables whose images ascend by id; a cap it finds exceeded is reported with the image's id where ``img_ids``
    (the tables' image ids, in table order) are given.  Returns (precision [T, R, K, A, M], recall [T, K, A, M]) on the device."""
    from . import ops  # registers the stlpose:: ops
    try:
        score, cat, rank, matched, ignored, npig = match()
    except ops.BoxApCapError as e:
        if img_ids is None:
            raise
        raise ValueError(f"image_id {int(img_ids[e.image_index])}: {e}") from None
    # one global order: stable by descending score, then stable by category.  The slots lie image by image (ascending ids) and rank
    # by rank within a category, so equal scores keep that order; slots of no category (-1) sort to the front and are skipped
    by_score = torch.sort(score, descending=True, stable=True).indices
    by_cat = torch.sort(cat[by_score], stable=True).indices
    order = by_score[by_cat]
    cat_offsets = torch.cumsum(torch.bincount((cat + 1).long(), minlength=num_cats + 1), 0)   # [K + 1]: where each category's slots begin
    return torch.ops.stlpose.box_ap_accumulate(matched, ignored, rank, order, cat_offsets, npig.sum(0, dtype=torch.int64), num_thrs,
                                               [int(m) for m in max_dets], [float(r) for r in REC_THRS])


def mean_valid(x: np.ndarray) -> float:
    """The mean of the entries > -1 (-1 marks "no ground truth to find"), or -1 without one."""
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0
