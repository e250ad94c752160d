"""The evaluation's per-batch tail without a host sync: ``Evaluator(tail="device")``.

``Evaluator._batch_outputs`` (the host tail) stops the device five or more times per batch: the loss's ``.item()``, two ``.cpu()``
of the PCK's arg-max, two of the decode.  ``EvalTables`` keeps what those copies carried -- per (person, joint) two arg-max
coordinates, the refined coordinates and the maximum, per batch one loss -- in tables on the device, filled by two launches per
batch (``stlpose::eval_tail``: csrc/eval_tail.hip, then ``stl_sum_partials``), and copies them to the host once, in ``finish``.
Every number equals the host tail's bit for bit, except the fp32 loss of a batch, which may be its float32 neighbour (the fp64
squared errors are summed in another order: see eval_tail.hip).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops  # noqa: F401  (registers the stlpose:: custom ops)
from .inference import _perm

NON_FINITE = ("stlpose_amd.Evaluator: non-finite heat maps.  With compute_dtype='mixed' (f16 forward tensors, |y| <= 65504) a "
              "badly scaled checkpoint overflows; evaluate it with compute_dtype='bf16' or 'fp32'.")


class EvalTables:
    """Epoch tables on the device: pred_xy, tgt_xy, coords float32 [rows, J, 2], maxval float32 [rows, J], losses float32 [batches].
    They start at ``ROWS`` rows (``BATCHES`` losses) and double when full: an allocation and a device copy on the current stream.
    ``add`` only lists launches; the one device->host copy of the epoch is in ``finish``."""
    ROWS, BATCHES = 4096, 256

    def __init__(self, device, joints: int = 17):
        self.device, self.joints = torch.device(device), int(joints)
        self.rows = self.batches = 0
        self.sizes: List[int] = []          # persons per batch
        self.hw: Optional[Tuple[int, int]] = None
        self._perm_host = _perm(self.joints, "cpu")   # uploaded without a blocking copy: the tables may be made inside the loop
        self._perm = self._perm_host.to(self.device, non_blocking=True)
        self._tables = self._alloc(self.ROWS)
        self._losses = torch.zeros(self.BATCHES, dtype=torch.float32, device=self.device)
        self._partial = torch.empty(0, dtype=torch.float64, device=self.device)
        self.preds: Optional[torch.Tensor] = None   # finish(): [N, J, 3] on the device

    def _alloc(self, rows: int):
        j = self.joints
        return [torch.zeros(rows, *tail, dtype=torch.float32, device=self.device) for tail in ((j, 2), (j, 2), (j, 2), (j,))]

    def _reserve(self, rows: int, batches: int) -> None:
        cap = self._tables[0].shape[0]
        if rows > cap:
            while cap < rows:
                cap *= 2
            new = self._alloc(cap)
            for n, o in zip(new, self._tables):
                n[:self.rows].copy_(o[:self.rows])
            self._tables = new
        if batches > self._losses.numel():
            new = torch.zeros(2 * self._losses.numel(), dtype=torch.float32, device=self.device)
            new[:self.batches].copy_(self._losses[:self.batches])
            self._losses = new

    def add(self, out: torch.Tensor, out_flipped: Optional[torch.Tensor], target: torch.Tensor, target_weight: torch.Tensor) -> None:
        """One batch: out, out_flipped (None: no flip test), target [B, J, H, W] and target_weight [B, J(, 1)] on the device."""
        b, j, h, w = out.shape
        if j != self.joints:
            raise ValueError(f"EvalTables: heat maps of {j} joints in tables of {self.joints}")
        if self.hw is None:
            self.hw = (h, w)
        elif self.hw != (h, w):
            raise ValueError(f"EvalTables: heat maps of {h} x {w} after maps of {self.hw[0]} x {self.hw[1]} in one epoch")
        self._reserve(self.rows + b, self.batches + 1)
        if self._partial.numel() < b * j:
            self._partial = torch.empty(b * j, dtype=torch.float64, device=self.device)
        torch.ops.stlpose.eval_tail(out, out_flipped, self._perm, target, target_weight, *self._tables, self._partial, self._losses,
                                    self.rows, self.batches)
        self.rows, self.batches = self.rows + b, self.batches + 1
        self.sizes.append(b)

    def finish(self, centers, scales, thr: float = 0.5):
        """centers, scales [N, 2] of all persons in the order they were added.  One ``eval_affine`` launch over the N rows, one
        device->host copy.  Returns (preds [N, J, 3] float32 numpy (x, y in image coordinates, maxval), the per-batch losses and
        the per-batch average PCK as lists of float); ``self.preds`` keeps the device tensor."""
        n, j = self.rows, self.joints
        centers, scales = np.asarray(centers, np.float32).reshape(-1, 2), np.asarray(scales, np.float32).reshape(-1, 2)
        if len(centers) != n or len(scales) != n:
            raise ValueError(f"EvalTables.finish: {len(centers)} centres and {len(scales)} scales for {n} persons")
        if n == 0:
            self.preds = torch.zeros(0, j, 3, dtype=torch.float32, device=self.device)
            return np.zeros((0, j, 3), np.float32), [], []
        from .pose_parsing import pck_from_coords
        h, w = self.hw
        pred_xy, tgt_xy, coords, maxval = self._tables
        cs = torch.from_numpy(np.concatenate([centers, scales], 1)).to(self.device)
        self.preds = torch.ops.stlpose.eval_affine(coords, maxval, cs[:, 0:2].contiguous(), cs[:, 2:4].contiguous(), h, w)
        # the epoch's only device -> host copy: [N, J, 7] = preds | pred_xy | tgt_xy, and the losses behind it
        packed = torch.cat([torch.cat([self.preds, pred_xy[:n], tgt_xy[:n]], 2).reshape(-1), self._losses[:self.batches]]).cpu().numpy()
        table, losses = packed[:n * j * 7].reshape(n, j, 7), packed[n * j * 7:]
        preds = np.ascontiguousarray(table[:, :, 0:3])
        if not np.isfinite(preds[:, :, 2]).all():
            raise FloatingPointError(NON_FINITE)
        pcks, r = [], 0
        for b in self.sizes:
            pcks.append(float(pck_from_coords(table[r:r + b, :, 3:5], table[r:r + b, :, 5:7], h, w, thr)[1]))
            r += b
        return preds, [float(v) for v in losses], pcks
