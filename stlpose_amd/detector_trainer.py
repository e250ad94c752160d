"""Fine-tuning the detector from COCO annotations: the loop of reference ``src/02_train_faster_rcnn.py:139-280`` over two
``det_data.DetBatchLoader``s, the detector's counterpart of ``trainer.Trainer``.

  * epoch structure ``:151-171``: validation epoch (``DetectorEvaluator.evaluate(valid_loader, gt, fraction=0.2)``: the first fifth of
    the loader, ``:254-256``; the ``GroundTruth`` is built once from ``DetectionDB.coco_gt``) -> training epoch -> scheduler step
    (``plateau`` steps on ``valid_ap``, as ``:157`` does) -> ``detector_logs.json`` -> checkpoint every ``save_frequency`` epochs, and
    ``checkpoint_epoch_final.pth`` at the end;
  * a training step ``:211-235``: ``loss_dict = model.detection_loss(batch)``, ``sum(loss_dict.values())``, ``apply_perceptual_loss``
    with the batch's ``perceptual_loss``, the skip of a zero or non-finite loss, ``zero_grad / backward / step``.  The skip reads the
    loss scalar: ONE host wait per step, as the reference has it (``loss.item()``, ``:220``); everything else of the step is enqueued
    without waiting;
  * ``setup_optimizer`` (``lib/model_setup.py:109-159``) over ``detector_train.trainable_parameters(model)`` -- the parameters
    ``detection_loss`` trains: the heads, and with ``exp_data["training"]["train_bifpn"] = k`` (default 0, applied to the model by
    ``set_train_bifpn``) the last k BiFPN cells, with ``"all"`` every cell, and with ``"all"`` and ``exp_data["training"]["train_backbone"] = k`` (default 0,
    ``set_train_backbone``) the last k MBConv blocks of the backbone's final stage, or instead with ``exp_data["training"]["train_trunk"] = k``
    (``set_train_trunk``; giving both keys is a ValueError) the last k blocks of the whole backbone, with ``"all"`` every block and the stem; everything before them is frozen: Adam, or SGD with momentum, nesterov and weight
    decay 0.0005;
    ``ReduceLROnPlateau(mode="max", min_lr=1e-8)``, ``StepLR`` or no scheduler;
  * ``detector_logs.json`` as ``create_ / load_ / update_detector_logs`` write it (``lib/utils.py:244-301``);
  * checkpoints ``<exp>/models/detector/checkpoint_epoch_{k|final}.pth`` with the four keys of ``save_checkpoint``
    (``model_setup.py:200-205``); ``load_checkpoint`` restores model, optimizer, scheduler and epoch (``:210-252``).  A resumed run
    continues with the epoch AFTER the one the checkpoint was written behind, so that it reaches the weights of the uninterrupted run
    (the reference restarts at ``checkpoint["epoch"]`` and trains that epoch a second time).

The model stays in ``eval()`` mode throughout: ``detection_loss`` keeps every BN on its running statistics whatever the mode is, and
the inference forward of the validation epoch refuses training mode.  Single process: data-parallel head training is out of scope
(``DetectorEvaluator`` alone takes a process group).
"""
from __future__ import annotations

import json
import math
import os
import time
from typing import Iterable, Optional

import numpy as np
import torch

from .detection_eval import DetectorEvaluator, GroundTruth
from .detector_train import trainable_parameters
from .loss import apply_perceptual_loss

LOGS_FILE = "detector_logs.json"


def _timestamp() -> str:
    return time.strftime("%Y-%m-%d_%H-%M-%S")


def create_detector_logs(exp_path: str) -> dict:
    logs = {"last_modified": _timestamp(), "train_loss": [], "valid_ap": []}
    with open(os.path.join(exp_path, LOGS_FILE), "w") as f:
        json.dump(logs, f)
    return logs


def load_detector_logs(exp_path: str) -> dict:
    with open(os.path.join(exp_path, LOGS_FILE)) as f:
        return json.load(f)


def update_detector_logs(exp_path: str, logs: dict, train_loss, valid_ap) -> None:
    logs["last_modified"] = _timestamp()
    logs["train_loss"].append(float(train_loss))
    logs["valid_ap"].append(float(valid_ap))
    with open(os.path.join(exp_path, LOGS_FILE), "w") as f:
        json.dump(logs, f)


def setup_optimizer(exp_data: dict, parameters):
    """lib/model_setup.py:109-159 over ``parameters``: (optimizer, scheduler or None)."""
    tr = exp_data["training"]
    parameters = list(parameters)
    if tr["optimizer"] == "adam":
        optimizer = torch.optim.Adam(parameters, lr=tr["learning_rate"])
    else:
        optimizer = torch.optim.SGD(parameters, lr=tr["learning_rate"], momentum=tr["momentum"], nesterov=tr["nesterov"],
                                    weight_decay=0.0005)
    kind = tr.get("scheduler", "plateau")
    if kind == "plateau":
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=tr["patience"], factor=tr["learning_rate_factor"],
                                                               min_lr=1e-8, mode="max")
    elif kind == "step":
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, gamma=tr["learning_rate_factor"], step_size=tr["patience"])
    else:
        scheduler = None
    return optimizer, scheduler


class DetectorTrainer:
    """``DetectorTrainer(exp_path, exp_data, model, train_loader, valid_loader, coco_gt).training_loop()``.

    model: an ``EfficientDetBackbone`` ("fp32" or "f16").  The loaders yield ``(DetBatch, metas)`` (``det_data.DetBatchLoader``); one
    with ``set_epoch`` is told the epoch before it is iterated, which is what makes a resumed run see the batches of the uninterrupted
    one.  coco_gt: ``db.coco_gt(image_size)`` of the validation table (or a ``GroundTruth``), uploaded once.  ``valid_fraction``: the
    share of the validation loader scored each epoch (the reference's fifth).  ``output``: ``DetectorEvaluator``'s."""

    def __init__(self, exp_path: str, exp_data: dict, model, train_loader: Iterable, valid_loader: Iterable, coco_gt,
                 checkpoint: Optional[str] = None, resume_training: bool = False, device="cuda", valid_fraction: float = 0.2,
                 output: str = "device", params=None):
        self.exp_path, self.exp_data, self.model = exp_path, exp_data, model
        self.train_loader, self.valid_loader = train_loader, valid_loader
        self.checkpoint, self.resume_training = checkpoint, bool(resume_training)
        self.device, self.valid_fraction, self.output = torch.device(device), float(valid_fraction), output
        self.params = params   # optional argparse-like object with .use_perceptual_loss
        tr = exp_data["training"]
        self.num_epochs, self.save_frequency = int(tr["num_epochs"]), int(tr["save_frequency"])
        self.scheduler_type = tr.get("scheduler", "plateau")
        self.cur_epoch, self.skipped = 0, 0
        self.train_loss, self.valid_ap, self.valid_stats = float("nan"), -1.0, None
        self.model.to(self.device).eval()
        k = tr.get("train_bifpn", 0)
        k = k if k == "all" else int(k)
        want = len(self.model.bifpn) if k == "all" else k
        if "train_trunk" in tr and "train_backbone" in tr:
            raise ValueError("DetectorTrainer: exp_data[\"training\"] has both train_backbone and train_trunk; give one (train_trunk reaches "
                             "every block, and with \"all\" the stem)")
        kb = int(tr.get("train_backbone", 0))   # the trailing MBConv blocks that train too: needs train_bifpn "all"
        kt = tr.get("train_trunk")              # the same without the final stage's limit (set_train_trunk), an int or "all"
        kt = None if kt is None else kt if kt == "all" else int(kt)
        none = kt == 0 if kt is not None else kb == 0
        if none and (getattr(self.model, "train_backbone", 0) or getattr(self.model, "train_stem", False)):
            self.model.set_train_backbone(0)
        if want != getattr(self.model, "train_bifpn", 0):   # (a model without that stage takes 0 only)
            self.model.set_train_bifpn(k)
        if kt is not None:
            if not none:
                self.model.set_train_trunk(kt)
        elif kb != getattr(self.model, "train_backbone", 0) or getattr(self.model, "train_stem", False):
            self.model.set_train_backbone(kb)
        self.optimizer, self.scheduler = setup_optimizer(exp_data, [p for _, p in trainable_parameters(model)])
        self.evaluator = DetectorEvaluator(model, device=self.device, output=output)
        self.gt = coco_gt if isinstance(coco_gt, GroundTruth) else self._ground_truth(coco_gt)
        os.makedirs(self.save_dir, exist_ok=True)
        if checkpoint is not None:
            self.load_checkpoint(checkpoint, only_model=not self.resume_training)

    def _ground_truth(self, coco_gt) -> GroundTruth:
        cats = [c["id"] for c in coco_gt["categories"]] if coco_gt.get("categories") else None
        return GroundTruth(coco_gt["annotations"], cats, device=self.device)

    @property
    def save_dir(self) -> str:
        return os.path.join(self.exp_path, "models", "detector")

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, epoch: int, finished: bool = False) -> str:
        name = "checkpoint_epoch_final.pth" if finished else f"checkpoint_epoch_{epoch}.pth"
        path = os.path.join(self.save_dir, name)
        torch.save({"epoch": epoch, "model_state_dict": {k: v.detach().cpu() for k, v in self.model.state_dict().items()},
                    "optimizer_state_dict": self.optimizer.state_dict(),
                    "scheduler_state_dict": self.scheduler.state_dict() if self.scheduler is not None else {}}, path)
        return path

    def load_checkpoint(self, path: str, only_model: bool = False) -> None:
        ck = torch.load(path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ck["model_state_dict"] if "model_state_dict" in ck else ck)
        if only_model:
            return
        self.optimizer.load_state_dict(ck["optimizer_state_dict"])
        if self.scheduler is not None and ck.get("scheduler_state_dict"):
            self.scheduler.load_state_dict(ck["scheduler_state_dict"])
        self.cur_epoch = int(ck["epoch"]) + 1   # the epoch behind which the checkpoint was written is done (module docstring)

    # ------------------------------------------------------------------ epochs
    def training_loop(self) -> None:
        if self.checkpoint is not None and self.resume_training:
            self.training_logs = load_detector_logs(self.exp_path)
        else:
            self.training_logs = create_detector_logs(self.exp_path)
        for epoch in range(self.cur_epoch, self.num_epochs):
            self.validation_epoch(epoch)
            self.train_epoch(epoch)
            if self.scheduler is not None:
                if self.scheduler_type == "plateau":
                    self.scheduler.step(self.valid_ap)
                else:
                    self.scheduler.step()
            update_detector_logs(self.exp_path, self.training_logs, self.train_loss, self.valid_ap)
            if epoch % self.save_frequency == 0:
                self.save_checkpoint(epoch)
        self.save_checkpoint(self.num_epochs, finished=True)

    def train_epoch(self, epoch: int) -> None:
        if hasattr(self.train_loader, "set_epoch"):
            self.train_loader.set_epoch(epoch)
        losses = []
        for batch, _metas in self.train_loader:
            loss_dict = self.model.detection_loss(batch)
            loss = sum(loss for loss in loss_dict.values())
            loss = apply_perceptual_loss(self.exp_data, self.params, loss, batch.perceptual_loss)
            loss_value = loss.item()   # the one host wait of the step
            if loss_value == 0 or not math.isfinite(loss_value):
                self.skipped += 1
                continue
            losses.append(loss_value)
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
        self.train_loss = float(np.mean(losses)) if losses else float("nan")

    def validation_epoch(self, epoch: int) -> None:
        if hasattr(self.valid_loader, "set_epoch"):
            self.valid_loader.set_epoch(epoch)
        res = self.evaluator.evaluate(self.valid_loader, self.gt, fraction=self.valid_fraction)
        self.valid_stats, self.valid_ap = [float(v) for v in res["stats"]], float(res["valid_ap"])
