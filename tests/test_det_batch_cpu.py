"""CPU: the host side of the detector's batch chain -- coco_detection_db on a hand-written COCO file, coco_gt, the numpy yardstick's
fixed points (tests/det_batch_ref.py), the refusals without a GPU, the new header as capi reads it, and DetectorTrainer's logs and
checkpoints with the model and the loaders replaced by stubs."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from stlpose_amd import capi, det_data, detector_trainer, ops
from stlpose_amd.det_data import DetBatchLoader, DetectionDB, coco_detection_db
from stlpose_amd.detection_eval import GroundTruth
from tests import det_batch_ref as R


# ------------------------------------------------------------------------------------------------ coco_detection_db
def _coco_file():
    """Three categories with non-contiguous ids (person = 7 is class 1, 3 is class 2, 90 is class 3) and five images."""
    ann = lambda i, img, cat, bbox, area, crowd=0: dict(id=i, image_id=img, category_id=cat, bbox=bbox, area=area, iscrowd=crowd)   # noqa: E731
    return {
        "categories": [{"id": 7, "name": "person"}, {"id": 3, "name": "cat"}, {"id": 90, "name": "kite"}],
        "images": [{"id": 42, "width": 100, "height": 80, "file_name": "a.jpg"}, {"id": 5, "width": 64, "height": 48, "file_name": "b.jpg"},
                   {"id": 9, "width": 30, "height": 40, "file_name": "c.jpg"}, {"id": 11, "width": 20, "height": 20, "file_name": "d.jpg"},
                   {"id": 77, "width": 50, "height": 60, "file_name": "e.jpg"}],
        "annotations": [
            ann(1, 42, 7, [10.5, 20.0, 30.0, 40.0], 1200.0),          # plain: x2 = 10.5 + 29 = 39.5, y2 = 20 + 39 = 59
            ann(2, 42, 7, [0.0, 0.0, 50.0, 50.0], 2500.0, crowd=1),   # crowd: dropped
            ann(3, 42, 7, [90.0, 70.0, 30.0, 30.0], 900.0),           # over the right and bottom edges: clipped to 99, 79
            ann(4, 5, 7, [12.0, 8.0, 0.0, 5.0], 3.0),                 # w = 0: kept, x2 == x1 = 12; y2 = 8 + 4 = 12
            ann(5, 5, 7, [1.0, 1.0, 10.0, 10.0], 0.0),                # area = 0: dropped
            ann(6, 9, 3, [2.0, 2.0, 10.0, 10.0], 100.0),              # a cat: dropped, and image 9 is left without a box
            ann(7, 77, 90, [5.0, 6.0, 7.0, 8.0], 56.0),               # a kite: class 3
            ann(8, 77, 7, [-3.0, -2.0, 10.0, 10.0], 50.0),            # negative corner: x1 = y1 = 0, x2 = y2 = 9
            ann(9, 42, 3, [1.0, 1.0, 5.0, 5.0], 25.0),                # a cat in image 42 (file order: after annotation 3)
        ]}


def test_coco_detection_db_rules():
    db = coco_detection_db(_coco_file())
    assert isinstance(db, DetectionDB) and len(db) == 3                # images 9 (no person) and 11 (no annotation) are dropped
    assert db.image_id.tolist() == [42, 5, 77] and db.image_id.dtype == np.int64
    assert db.file_name == ["000000000042.jpg", "000000000005.jpg", "000000000077.jpg"] == db.original_name
    assert db.height.tolist() == [80, 48, 60] and db.width.tolist() == [100, 64, 50] and db.height.dtype == np.int32
    assert db.box_start.tolist() == [0, 2, 3] and db.box_count.tolist() == [2, 1, 1]
    assert db.box_start.dtype == np.int64 and db.box_count.dtype == np.int32
    want = np.array([[10.5, 20, 39.5, 59], [90, 70, 99, 79], [12, 8, 12, 12], [0, 0, 9, 9]], np.float32)
    assert db.boxes.dtype == np.float32 and np.array_equal(db.boxes, want)
    assert db.labels.tolist() == [1, 1, 1, 1] and db.labels.dtype == np.int64
    assert db.area.tolist() == [1200.0, 900.0, 3.0, 50.0] and db.area.dtype == np.float64
    assert db.perceptual_loss.tolist() == [0.0, 0.0, 0.0]
    assert db.image_sizes() == [(80, 100), (48, 64), (60, 50)]


def test_coco_detection_db_class_ids_by_position():
    db = coco_detection_db(_coco_file(), class_ids=[2, 3])             # cat (id 3) is class 2, kite (id 90) is class 3
    assert db.image_id.tolist() == [42, 9, 77]
    assert db.labels.tolist() == [2, 2, 3] and db.box_count.tolist() == [1, 1, 1]
    assert np.array_equal(db.boxes, np.array([[1, 1, 5, 5], [2, 2, 11, 11], [5, 6, 11, 13]], np.float32))
    both = coco_detection_db(_coco_file(), class_ids=[1, 3])
    assert both.labels.tolist() == [1, 1, 1, 3, 1] and both.box_start.tolist() == [0, 2, 3]   # file order inside image 77


def test_coco_detection_db_styled_names_and_perceptual_loss(tmp_path):
    mapping = {"000000000042": "s42_alpha_0.5.jpg", "000000000005": "s5.jpg", "000000000077": "s77.jpg"}
    perc = {"s42_alpha_0.5.jpg": 0.25, "s5.jpg": 1.5, "s77.jpg": 0.0, "unused.jpg": 9.0}
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(_coco_file()))
    db = coco_detection_db(str(path), mapping=mapping, perceptual_loss=perc)
    assert db.file_name == ["s42_alpha_0.5.jpg", "s5.jpg", "s77.jpg"]
    assert db.original_name == ["000000000042.jpg", "000000000005.jpg", "000000000077.jpg"]
    assert db.perceptual_loss.tolist() == [0.25, 1.5, 0.0]
    with pytest.raises(KeyError):
        coco_detection_db(_coco_file(), mapping={"000000000042": "x.jpg"})


def test_coco_gt_is_what_the_evaluator_takes():
    db = coco_detection_db(_coco_file(), class_ids=[1, 3])
    gt = db.coco_gt(50)
    scale = {42: np.float32(50 / 100), 5: np.float32(50 / 64), 77: np.float32(50 / 60)}   # S1 / the longer side
    anns = gt["annotations"]
    assert [a["id"] for a in anns] == [1, 2, 3, 4, 5] and [a["image_id"] for a in anns] == [42, 42, 5, 77, 77]
    assert [a["category_id"] for a in anns] == [1, 1, 1, 3, 1] and all(a["iscrowd"] == 0 for a in anns)
    assert [a["area"] for a in anns] == [1200.0, 900.0, 3.0, 56.0, 50.0]                   # the file's, unscaled
    for a, box in zip(anns, db.boxes):
        b = (box * scale[a["image_id"]]).astype(np.float32)
        want = [b[0], b[1], np.float32(b[2] - b[0]), np.float32(b[3] - b[1])]              # xywh by the float32 subtraction
        assert a["bbox"] == [float(v) for v in want]
    assert gt["categories"] == [{"id": 1}, {"id": 3}]
    assert gt["images"] == [{"id": i, "height": 50, "width": 50} for i in (42, 5, 77)]
    table = GroundTruth(gt["annotations"], [c["id"] for c in gt["categories"]], device="cpu")
    assert table.img_ids.tolist() == [5, 42, 77] and table.counts.tolist() == [1, 2, 2] and table.cat_ids == [1, 3]
    assert np.array_equal(db.scaled_boxes(50)[:2], (db.boxes[:2] * np.float32(0.5)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the yardstick's fixed points
def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_yardstick_sizes_follow_the_reference():
    assert R.resized_size(17, 29, 24)[1:] == (int(17 * (24 / 29)), 24)
    assert R.resized_size(40, 23, 24)[1:] == (24, int(23 * (24 / 40)))
    assert R.resized_size(31, 31, 24)[1:] == (int(31 * (24 / 31)), 24)    # the tie takes the else branch: the width is S1
    assert R.resized_size(480, 640, 512) == (0.8, 384, 512)
    for h, w in ((17, 29), (40, 23), (31, 31), (10, 24), (480, 640)):
        assert R.resized_size(h, w, 24) == det_data.resized_size(h, w, 24)


def test_yardstick_identity_constant_and_double_flip():
    img = _image(10, 24, 1)                                              # already S1 on its longer side
    out = R.stage1(img, 24)
    assert np.array_equal(out[:10], img) and not out[10:].any()
    tall = _image(24, 7, 2)
    assert np.array_equal(R.stage1(tall, 24)[:, :7], tall) and not R.stage1(tall, 24)[:, 7:].any()
    const = np.full((40, 23, 3), (200, 17, 3), np.uint8)
    out = R.stage1(const, 24)
    _, rh, rw = R.resized_size(40, 23, 24)
    assert (rh, rw) == (24, 13) and (out[:rh, :rw] == np.array([200, 17, 3], np.uint8)).all() and not out[:, rw:].any()
    for h, w in ((17, 29), (40, 23), (31, 31)):
        img = _image(h, w, h)
        _, rh, rw = R.resized_size(h, w, 24)
        once = R.stage1(img, 24, flip=True)
        assert np.array_equal(once[:rh, :rw][:, ::-1], R.stage1(img, 24)[:rh, :rw]) and not once[rh:].any() and not once[:, rw:].any()
        boxes = np.array([[1.5, 2.0, 9.25, 11.0]], np.float32)
        fb = R.scaled_boxes(boxes, h, w, 24, flip=True)
        sb = R.scaled_boxes(boxes, h, w, 24)
        assert fb[0, 0] == np.float32(rw - 1) - sb[0, 2] and fb[0, 2] == np.float32(rw - 1) - sb[0, 0] and fb[0, 0] <= fb[0, 2]
        assert np.array_equal(fb[:, [1, 3]], sb[:, [1, 3]])


def test_yardstick_gt_table_is_pack_targets():
    """The table the kernel writes is, by definition, pack_targets on the scaled boxes of S1 x S1 images."""
    from stlpose_amd.detector_train import pack_targets
    from stlpose_amd.efficientdet import resize_meta
    sizes = [(17, 29), (40, 23), (31, 31), (24, 10)]
    boxes = [np.array([[1, 2, 9, 11], [0, 0, 28, 16], [3.5, 4.25, 7.75, 8.5]], np.float32), np.zeros((0, 4), np.float32),
             np.array([[2, 3, 30, 30]], np.float32), np.array([[0, 0, 5, 5], [1, 2, 8, 20]], np.float32)]
    labels = [[1, 2, 1], [], [1], [2, 1]]
    for s1, s in ((24, 32), (32, 32), (400, 512)):
        new_w, new_h = resize_meta(s1, s1, s)[:2]
        gt, off = R.gt_table(boxes, labels, sizes, s1, new_w / s1, new_h / s1)
        targets = [dict(boxes=torch.from_numpy(R.scaled_boxes(b, h, w, s1)), labels=torch.tensor(l, dtype=torch.int64))
                   for b, l, (h, w) in zip(boxes, labels, sizes)]
        if s == 512:   # pack_targets is written for the 512 canvas
            want_gt, want_off = pack_targets(targets, [(s1, s1)] * 4, 2)
            assert np.array_equal(gt, want_gt) and np.array_equal(off, want_off)
        assert off.tolist() == [0, 3, 3, 4, 6] and gt.dtype == np.float32 and gt[:, 4].tolist() == [0, 1, 0, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ no GPU, no batches
class _Store:
    device_resident = True

    def __len__(self):
        return 3


def test_loader_refuses_a_cpu_device():
    db = coco_detection_db(_coco_file())
    with pytest.raises(RuntimeError, match=r"DetBatchLoader \(HIP\) needs a GPU device; there is no CPU path"):
        DetBatchLoader(db, _Store(), None, 2, True, image_size=24, device="cpu")


def test_op_has_no_cpu_kernel():
    assert "det_batch" in ops.OPS
    i64, i32 = torch.int64, torch.int32
    args = (torch.zeros(1, 32, 32, 3), torch.zeros(300, dtype=torch.uint8), torch.zeros(1, dtype=i64), torch.tensor([[10, 10]], dtype=i32),
            torch.zeros(1, dtype=i64), torch.zeros(1, dtype=i64), torch.ones(1, dtype=i32), torch.zeros(1, 4), torch.ones(1, dtype=i64))
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.stlpose.det_batch(*args, None, False, 24, 1, False)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        dev = dict(device="cuda")
        s1, gt, off = torch.ops.stlpose.det_batch(
            torch.empty(2, 32, 32, 3, **dev), torch.empty(600, dtype=torch.uint8, **dev), torch.empty(2, dtype=i64, **dev),
            torch.empty(2, 2, dtype=i32, **dev), torch.empty(2, dtype=i64, **dev), torch.empty(5, dtype=i64, **dev),
            torch.empty(5, dtype=i32, **dev), torch.empty(9, 4, **dev), torch.empty(9, dtype=i64, **dev), None, False, 24, 3, True)
        assert s1.shape == (2, 24, 24, 3) and s1.dtype == torch.uint8 and gt.shape == (3, 5) and off.shape == (3,) and off.dtype == i32


def test_det_batch_header_is_read():
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    h = capi.DET_BATCH
    assert h.signatures == {"stl_det_batch": [vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp]}
    assert h.restypes == {"stl_det_batch": C.c_int} and h.structs == {}
    assert h.constants == {"STL_DET_BATCH_MAX": 1024, "STL_DET_BATCH_SIDE": 4096}
    assert capi.DET_BATCH_MAX == 1024 and capi.DET_BATCH_SIDE == 4096
    assert not set(h.signatures) & (set(capi.SIGNATURES) | set(capi.DETECTIONS.signatures))


# ------------------------------------------------------------------------------------------------ DetectorTrainer on stubs
class _Head(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(3))


class _StubModel(torch.nn.Module):
    """detection_loss is a quadratic in the head parameters times the batch's value: enough for an optimiser to move them."""

    def __init__(self):
        super().__init__()
        self.regressor, self.classifier, self.trunk = _Head(1), _Head(2), torch.nn.Linear(2, 2)

    def detection_loss(self, batch):
        return {"classification": (self.classifier.w ** 2).sum() * batch.value, "regression": (self.regressor.w ** 2).sum() * batch.value}


class _StubBatch:
    def __init__(self, value):
        self.value, self.perceptual_loss = value, torch.tensor([0.5, 1.5], dtype=torch.float64)


class _StubLoader:
    def __init__(self, values):
        self.values, self.epochs = values, []

    def set_epoch(self, epoch):
        self.epochs.append(epoch)

    def __len__(self):
        return len(self.values)

    def __iter__(self):
        return iter([(_StubBatch(v), [{"image_id": 1}, {"image_id": 2}]) for v in self.values])


class _StubEvaluator:
    def __init__(self):
        self.calls = []

    def evaluate(self, loader, gt, fraction=1.0):
        self.calls.append(fraction)
        ap = 0.125 * len(self.calls)
        return {"stats": np.full(12, ap), "valid_ap": ap}


def _exp_data(**training):
    tr = {"num_epochs": 3, "save_frequency": 2, "learning_rate": 0.1, "learning_rate_factor": 0.5, "patience": 1, "momentum": 0.9,
          "optimizer": "sgd", "nesterov": True, "scheduler": "plateau", "perceptual_loss": False}
    tr.update(training)
    return {"training": tr, "dataset": {"dataset_name": "coco"}}


def _trainer(tmp_path, exp_data, values=(1.0, 2.0, float("nan"), 0.0), **kw):
    gt = {"annotations": [dict(image_id=1, category_id=1, bbox=[0, 0, 5, 5], area=25.0, iscrowd=0, id=1)], "categories": [{"id": 1}]}
    t = detector_trainer.DetectorTrainer(str(tmp_path), exp_data, _StubModel(), _StubLoader(list(values)), _StubLoader([1.0]), gt,
                                         device="cpu", **kw)
    t.evaluator = _StubEvaluator()
    return t


def test_trainer_logs_checkpoints_and_skips(tmp_path):
    t = _trainer(tmp_path, _exp_data())
    assert isinstance(t.optimizer, torch.optim.SGD) and t.optimizer.defaults["weight_decay"] == 0.0005 and t.optimizer.defaults["nesterov"]
    assert isinstance(t.scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau) and t.scheduler.mode == "max" and t.scheduler.min_lrs == [1e-8]
    assert sum(p.numel() for g in t.optimizer.param_groups for p in g["params"]) == 6          # the two heads, not the trunk
    trunk0 = t.model.trunk.weight.detach().clone()
    head0 = t.model.regressor.w.detach().clone()
    t.training_loop()
    logs = json.loads((tmp_path / "detector_logs.json").read_text())
    assert sorted(logs) == ["last_modified", "train_loss", "valid_ap"]
    assert logs["valid_ap"] == [0.125, 0.25, 0.375] and len(logs["train_loss"]) == 3 and all(np.isfinite(logs["train_loss"]))
    assert t.evaluator.calls == [0.2, 0.2, 0.2] and t.skipped == 6                              # the NaN and the zero loss of each epoch
    assert t.train_loader.epochs == [0, 1, 2]
    saved = sorted(os.listdir(tmp_path / "models" / "detector"))
    assert saved == ["checkpoint_epoch_0.pth", "checkpoint_epoch_2.pth", "checkpoint_epoch_final.pth"]
    ck = torch.load(tmp_path / "models" / "detector" / "checkpoint_epoch_2.pth", weights_only=False)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"] and ck["epoch"] == 2
    final = torch.load(tmp_path / "models" / "detector" / "checkpoint_epoch_final.pth", weights_only=False)
    assert final["epoch"] == 3 and torch.equal(final["model_state_dict"]["regressor.w"], t.model.regressor.w.detach())
    assert torch.equal(t.model.trunk.weight, trunk0) and not torch.equal(t.model.regressor.w.detach(), head0)
    assert torch.isfinite(t.model.regressor.w).all()                                           # the NaN batch was skipped, not stepped


def test_trainer_resumes_behind_the_saved_epoch(tmp_path):
    full = _trainer(tmp_path / "full", _exp_data(save_frequency=1, optimizer="adam", scheduler="step"))
    os.makedirs(tmp_path / "full", exist_ok=True)
    full.training_loop()
    ck = str(tmp_path / "full" / "models" / "detector" / "checkpoint_epoch_0.pth")
    os.makedirs(tmp_path / "resumed", exist_ok=True)
    (tmp_path / "resumed" / "detector_logs.json").write_text(json.dumps({"last_modified": "", "train_loss": [7.0], "valid_ap": [0.5]}))
    res = _trainer(tmp_path / "resumed", _exp_data(save_frequency=1, optimizer="adam", scheduler="step"), checkpoint=ck,
                   resume_training=True)
    assert res.cur_epoch == 1 and isinstance(res.optimizer, torch.optim.Adam) and isinstance(res.scheduler, torch.optim.lr_scheduler.StepLR)
    res.training_loop()
    assert res.train_loader.epochs == [1, 2]
    for k, v in full.model.state_dict().items():
        assert torch.equal(v, res.model.state_dict()[k]), k
    logs = json.loads((tmp_path / "resumed" / "detector_logs.json").read_text())
    assert len(logs["train_loss"]) == 3 and logs["train_loss"][0] == 7.0                       # the loaded logs are continued
    fresh = _trainer(tmp_path / "tuned", _exp_data(scheduler="none"), checkpoint=ck)           # fine-tuning: the weights alone
    assert fresh.cur_epoch == 0 and fresh.scheduler is None


def test_trainer_applies_the_perceptual_loss(tmp_path):
    exp = _exp_data(num_epochs=1, perceptual_loss=True, scheduler="none")
    exp["dataset"]["dataset_name"] = "styled_coco"
    with_p = _trainer(tmp_path / "p", exp, values=(1.0,))
    os.makedirs(tmp_path / "p", exist_ok=True)
    with_p.training_loop()
    plain = _trainer(tmp_path / "q", _exp_data(num_epochs=1, scheduler="none"), values=(1.0,))
    os.makedirs(tmp_path / "q", exist_ok=True)
    plain.training_loop()
    assert with_p.train_loss == pytest.approx(plain.train_loss * 2.0)                          # loss + loss * mean(0.5, 1.5)
