"""GPU: stlpose::det_batch against the numpy yardstick (tests/det_batch_ref.py) and against stl_det_preprocess, the kernel whose work
it fuses; EfficientDetBackbone on a DetBatch against the host-fed path; DetBatchLoader (what it yields, that it repeats, that it does
not wait for the device); and DetectorTrainer end to end.  Every comparison is exact."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stlpose_amd  # noqa: E402,F401  (registers the stlpose:: ops)
from stlpose_amd import capi, det_data, efficientdet as E, ops  # noqa: E402
from stlpose_amd.det_data import DetBatch, DetBatchLoader, DetectionDB  # noqa: E402
from stlpose_amd.detector_train import head_parameters  # noqa: E402
from stlpose_amd.detector_trainer import DetectorTrainer  # noqa: E402
from stlpose_amd.pose_data import ResidentImages, StreamedImages, epoch_indices  # noqa: E402
from tests import det_batch_ref as R, detector_ref as DR  # noqa: E402

DEV = "cuda"
# (height, width): landscape, portrait, the tie (the reference's else branch), and one already 24 wide (stage-1 identity at S1 = 24)
OP_SIZES = [(17, 29), (40, 23), (31, 31), (10, 24)]
OP_BOXES = [np.array([[1, 2, 9, 11], [0, 0, 28, 16], [3.5, 4.25, 7.75, 8.5]], np.float32), np.zeros((0, 4), np.float32),
            np.array([[2, 3, 30, 30]], np.float32), np.array([[0, 0, 5, 5], [1.125, 2, 8, 9]], np.float32)]
OP_LABELS = [[1, 2, 1], [], [1], [2, 1]]


def _images(sizes, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _db(sizes, boxes, labels, first_id=100) -> DetectionDB:
    counts = np.asarray([len(l) for l in labels], np.int32)
    n = len(sizes)
    return DetectionDB(image_id=first_id + np.arange(n, dtype=np.int64), file_name=[f"s{k}.jpg" for k in range(n)],
                       original_name=["%012d.jpg" % (first_id + k) for k in range(n)],
                       height=np.asarray([h for h, _ in sizes], np.int32), width=np.asarray([w for _, w in sizes], np.int32),
                       perceptual_loss=np.arange(n) / 8.0, box_start=(np.cumsum(counts) - counts).astype(np.int64), box_count=counts,
                       boxes=np.concatenate(boxes).astype(np.float32).reshape(-1, 4),
                       labels=np.asarray([v for l in labels for v in l], np.int64), area=np.ones(int(counts.sum())))


def _preprocess(stage1: np.ndarray, s: int) -> torch.Tensor:
    """stl_det_preprocess on the stage-1 images as float CHW / 255 (divided on the host, as the reference's dataset does it)."""
    b, s1 = stage1.shape[0], stage1.shape[1]
    chw = torch.from_numpy(stage1.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).contiguous().to(DEV)
    new_w, new_h = E.resize_meta(s1, s1, s)[:2]
    recs = (capi.DetImage * b)()
    for i in range(b):
        recs[i] = capi.DetImage(chw[i].data_ptr(), 1, s1, s1, new_h, new_w, 0, 1.0 / (new_h / s1), 1.0 / (new_w / s1))
    tab = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)
    out = torch.full((b, s, s, 3), float("nan"), device=DEV)
    capi.call("stl_det_preprocess", tab.data_ptr(), b, s, out.data_ptr(), ops._st())
    torch.cuda.synchronize()
    return out.cpu()


def _run_op(images, db, index, s1, s, draws=None, flip=False):
    store = ResidentImages.from_arrays(images, DEV)
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    rows = store.rows(idx.clamp(0, len(images) - 1))
    valid = [k for k in index if 0 <= k < len(db)]
    d = None if draws is None else torch.tensor(draws, dtype=torch.float64, device=DEV)
    return det_data.det_batch(rows, idx, db.device_tables(DEV), d, flip, s1, int(db.box_count[valid].sum()), s, stage1=True)


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("s1,s,flips", [(24, 32, None), (32, 32, None), (24, 32, (True, False, True, False))])
def test_op_matches_yardstick_and_the_kernel_it_fuses(s1, s, flips):
    images, db = _images(OP_SIZES), _db(OP_SIZES, OP_BOXES, OP_LABELS)
    draws = None if flips is None else [0.25 if f else 0.75 for f in flips]
    batch = _run_op(images, db, [0, 1, 2, 3], s1, s, draws, flips is not None)
    want1 = np.stack([R.stage1(im, s1, bool(flips[i]) if flips else False) for i, im in enumerate(images)])
    got1 = batch.stage1.cpu().numpy()
    assert got1.dtype == np.uint8 and np.array_equal(got1, want1)
    if s1 == 24 and flips is None:
        assert np.array_equal(got1[3, :10], images[3])                      # already S1 wide: the image itself
    new_w, new_h = E.resize_meta(s1, s1, s)[:2]
    gt, off = R.gt_table(OP_BOXES, OP_LABELS, OP_SIZES, s1, new_w / s1, new_h / s1, flips)
    assert batch.offsets.dtype == torch.int32 and batch.offsets.cpu().tolist() == off.tolist() == [0, 3, 3, 4, 6]
    assert batch.gt.dtype == torch.float32 and np.array_equal(batch.gt.cpu().numpy(), gt)
    assert batch.meta == E.resize_meta(s1, s1, s) and batch.image_size == s1
    canvas = batch.canvas.cpu()
    assert tuple(canvas.shape) == (4, s, s, 3) and torch.equal(canvas, _preprocess(want1, s))
    again = _run_op(images, db, [0, 1, 2, 3], s1, s, draws, flips is not None)  # a pure function of its inputs
    assert torch.equal(again.canvas, batch.canvas) and torch.equal(again.gt, batch.gt) and torch.equal(again.stage1, batch.stage1)


def test_op_draws_without_the_switch_do_not_flip():
    images, db = _images(OP_SIZES), _db(OP_SIZES, OP_BOXES, OP_LABELS)
    plain = _run_op(images, db, [0, 1, 2, 3], 24, 32)
    off = _run_op(images, db, [0, 1, 2, 3], 24, 32, [0.1] * 4, False)
    assert torch.equal(plain.canvas, off.canvas) and torch.equal(plain.gt, off.gt) and torch.equal(plain.stage1, off.stage1)


def test_op_reads_nothing_for_an_index_outside_the_table():
    images, db = _images(OP_SIZES), _db(OP_SIZES, OP_BOXES, OP_LABELS)
    s1, s = 24, 32
    batch = _run_op(images, db, [3, -1, len(db) + 3, 0], s1, s)
    good = _run_op(images, db, [3, 0], s1, s)
    canvas = batch.canvas.cpu()
    assert not canvas[1].any() and not canvas[2].any() and not batch.stage1[1:3].any()
    assert torch.equal(canvas[[0, 3]], good.canvas.cpu()) and torch.equal(batch.stage1[[0, 3]], good.stage1)
    assert batch.offsets.cpu().tolist() == [0, 2, 2, 2, 5] and torch.equal(batch.gt, good.gt)


def test_op_checks_its_arguments():
    images, db = _images(OP_SIZES), _db(OP_SIZES, OP_BOXES, OP_LABELS)
    store = ResidentImages.from_arrays(images, DEV)
    idx = torch.arange(4, device=DEV)
    src, off, hw = store.rows(idx)
    tabs = db.device_tables(DEV)
    canvas = torch.empty(4, 32, 32, 3, device=DEV)
    op = torch.ops.stlpose.det_batch
    for args in ((canvas[:3], src, off, hw, idx, *tabs), (canvas, src.float(), off, hw, idx, *tabs), (canvas, src, off.int(), hw, idx, *tabs),
                 (canvas, src, off, hw.long(), idx, *tabs), (canvas, src, off, hw, idx.int(), *tabs),
                 (canvas, src, off, hw, idx, tabs[0], tabs[1].long(), tabs[2], tabs[3]),
                 (canvas, src, off, hw, idx, tabs[0], tabs[1], tabs[2].double(), tabs[3]),
                 (canvas.double(), src, off, hw, idx, *tabs), (torch.empty(4, 32, 16, 3, device=DEV), src, off, hw, idx, *tabs)):
        with pytest.raises(ValueError, match="det_batch"):
            op(*args, None, False, 24, 6, False)
    with pytest.raises(ValueError, match="draws"):
        op(canvas, src, off, hw, idx, *tabs, torch.zeros(3, dtype=torch.float64, device=DEV), True, 24, 6, False)
    with pytest.raises(ValueError, match="S1"):
        op(canvas, src, off, hw, idx, *tabs, None, False, capi.DET_BATCH_SIDE + 1, 6, False)


# ------------------------------------------------------------------------------------------------ the model on a DetBatch
CLS_HEADER_SCALE, CLS_HEADER_BIAS = 0.1, -2.0   # the training tests' classifier header (test_detector_train_gpu.py): inside the loss's clamp
MODEL_BOXES = [np.array([[60.0, 40.0, 180.0, 160.0], [300.0, 30.0, 331.0, 61.0]], np.float32), np.zeros((0, 4), np.float32)]
MODEL_LABELS = [[1, 1], []]


def _model(compute_dtype="fp32", train_header=False):
    m = E.setup_detector("efficientdet", "d0", compute_dtype=compute_dtype)
    sd = DR.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    if train_header:
        sd["classifier.header.pointwise_conv.conv.weight"] = sd["classifier.header.pointwise_conv.conv.weight"] * CLS_HEADER_SCALE
        sd["classifier.header.pointwise_conv.conv.bias"] = torch.full_like(sd["classifier.header.pointwise_conv.conv.bias"], CLS_HEADER_BIAS)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def detector():
    return _model()


@pytest.fixture(scope="module")
def trainable():
    return _model(train_header=True)


def _model_batch(s1):
    images = DR.images()                                                     # 300 x 400 and 480 x 360
    sizes = [im.shape[:2] for im in images]
    db = _db(sizes, MODEL_BOXES, MODEL_LABELS)
    batch = _run_op(images, db, [0, 1], s1, E.MAX_SIZE)
    x = torch.from_numpy(batch.stage1.cpu().numpy().transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).to(DEV)
    targets = [dict(boxes=torch.from_numpy(R.scaled_boxes(b, h, w, s1)), labels=torch.tensor(l, dtype=torch.int64))
               for b, l, (h, w) in zip(MODEL_BOXES, MODEL_LABELS, sizes)]
    return batch, x, targets


def _same_list(a, b):
    assert len(a) == len(b)
    for da, db_ in zip(a, b):
        for k in ("boxes", "labels", "scores"):
            assert da[k].dtype == db_[k].dtype and torch.equal(da[k], db_[k]), k


@pytest.mark.parametrize("s1", [400, 512])
def test_model_detects_on_a_batch_as_on_the_host_fed_images(detector, s1):
    batch, x, _ = _model_batch(s1)
    got = detector(batch)
    want = detector(x)
    assert sum(len(d["scores"]) for d in want) > 0
    _same_list(got, want)
    dev_got, dev_want = detector(batch, output="device"), detector(x, output="device")
    assert torch.equal(dev_got.count, dev_want.count) and int(dev_want.count.min()) >= 0
    _same_list(dev_got.to_list(), dev_want.to_list())
    _same_list(dev_got.to_list(), want)
    feats, reg, cls, _ = detector(batch, postprocess=False)
    feats_w, reg_w, cls_w, _ = detector(x, postprocess=False)
    assert torch.equal(reg, reg_w) and torch.equal(cls, cls_w) and all(torch.equal(a, b) for a, b in zip(feats, feats_w))


def _loss_and_grads(m, *args):
    for _, p in head_parameters(m):
        p.grad = None
    out = m.detection_loss(*args)
    (out["classification"] + out["regression"]).backward()
    return out["classification"].detach().clone(), out["regression"].detach().clone(), {n: p.grad.clone() for n, p in head_parameters(m)}


def _check_loss(m, s1):
    batch, x, targets = _model_batch(s1)
    c, r, g = _loss_and_grads(m, batch)
    cw, rw, gw = _loss_and_grads(m, x, targets)
    print(f"S1 {s1} {m.compute_dtype}: classification {float(c):.6f} regression {float(r):.6f}")
    assert float(c) > 0 and float(r) > 0 and torch.isfinite(c) and torch.isfinite(r)
    assert torch.equal(c, cw) and torch.equal(r, rw)
    assert sorted(g) == sorted(gw) and len(g) > 0
    for n in g:
        assert torch.equal(g[n], gw[n]), n
    assert any(bool(v.any()) for v in g.values())
    with pytest.raises(ValueError, match="carries its targets"):
        m.detection_loss(batch, targets)


@pytest.mark.parametrize("s1", [400, 512])
def test_detection_loss_on_a_batch_equals_the_host_fed_one(trainable, s1):
    _check_loss(trainable, s1)


def test_detection_loss_on_a_batch_f16():
    _check_loss(_model("f16", train_header=True), 400)


# ------------------------------------------------------------------------------------------------ the loader
L_SIZES = [(40, 56), (64, 48), (50, 50), (33, 70), (72, 31)]
L_BOXES = [np.array([[4, 5, 30, 31], [10, 2, 50, 20]], np.float32), np.array([[1, 1, 40, 60]], np.float32),
           np.array([[5, 5, 45, 45], [0, 0, 10, 10], [20, 20, 49, 49]], np.float32), np.array([[3, 3, 60, 30]], np.float32),
           np.array([[2, 8, 28, 70], [0, 0, 30, 71]], np.float32)]
L_LABELS = [[1, 1], [1], [1, 1, 1], [1], [1, 1]]


def _loader(is_train, store=ResidentImages, exp_data=None, **kw):
    images, db = _images(L_SIZES, 11), _db(L_SIZES, L_BOXES, L_LABELS)
    kw.setdefault("canvas_size", 64)
    return DetBatchLoader(db, store.from_arrays(images, DEV), exp_data, 2, is_train, image_size=48, seed=5, stage1=True, **kw), images, db


def _tensors(batch):
    return batch.canvas, batch.gt, batch.offsets, batch.stage1


def test_loader_repeats_an_epoch_and_shuffles_the_next():
    loader, images, db = _loader(True)
    assert len(loader) == 2
    first = [(b, m) for b, m in loader]                                       # epoch 0
    loader.set_epoch(0)
    second = [(b, m) for b, m in loader]
    third = [(b, m) for b, m in loader]                                       # epoch 1
    assert len(first) == len(second) == len(third) == 2
    for (a, ma), (b, mb) in zip(first, second):
        assert ma == mb and all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))
    order = lambda e: [int(k) for rows in epoch_indices(5, 2, 5, e) for k in rows]   # noqa: E731
    assert order(0) != order(1)
    assert [m["image_id"] - 100 for _, ms in first for m in ms] == order(0)
    assert [m["image_id"] - 100 for _, ms in third for m in ms] == order(1)
    batch, metas = first[0]
    rows = [m["image_id"] - 100 for m in metas]
    assert isinstance(batch, DetBatch) and len(batch) == 2 and tuple(batch.canvas.shape) == (2, 64, 64, 3)
    want1 = np.stack([R.stage1(images[k], 48) for k in rows])
    assert np.array_equal(batch.stage1.cpu().numpy(), want1) and torch.equal(batch.canvas.cpu(), _preprocess(want1, 64))
    new_w, new_h = E.resize_meta(48, 48, 64)[:2]
    gt, off = R.gt_table([L_BOXES[k] for k in rows], [L_LABELS[k] for k in rows], [L_SIZES[k] for k in rows], 48, new_w / 48, new_h / 48)
    assert np.array_equal(batch.gt.cpu().numpy(), gt) and batch.offsets.cpu().tolist() == off.tolist()
    k = rows[0]
    assert metas[0] == {"image_id": 100 + k, "image_name": f"s{k}.jpg", "original_image_name": "%012d.jpg" % (100 + k),
                        "scale": R.resized_size(*L_SIZES[k], 48)[0], "original_size": L_SIZES[k], "perceptual_loss": k / 8.0}
    assert batch.perceptual_loss.tolist() == [r / 8.0 for r in rows] and torch.equal(loader.last["index"].cpu(), torch.tensor(order(1)[2:4]))


def test_validation_loader_keeps_the_table_order_and_the_ragged_tail():
    loader, images, db = _loader(False)
    assert len(loader) == 3
    batches = list(loader)
    assert [[m["image_id"] for m in ms] for _, ms in batches] == [[100, 101], [102, 103], [104]]
    tail, _ = batches[2]
    assert len(tail) == 1 and tail.offsets.cpu().tolist() == [0, 2] and tuple(tail.gt.shape) == (2, 5)
    assert batches[1][0].offsets.cpu().tolist() == [0, 3, 4]
    for i, (b, ms) in enumerate(batches):                                     # indexable, as DetectorEvaluator shards it
        again, ms2 = loader[i]
        assert ms2 == ms and all(torch.equal(x, y) for x, y in zip(_tensors(again), _tensors(b)))
    with pytest.raises(IndexError):
        loader[3]
    streamed, _, _ = _loader(False, StreamedImages)
    for (a, ma), (b, mb) in zip(streamed, batches):
        assert ma == mb and all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))


def test_training_loader_flips_by_its_draws():
    exp_data = {"dataset": {"flip": True, "dataset_name": "coco"}}
    loader, images, db = _loader(True, exp_data=exp_data)
    valid, _, _ = _loader(False, exp_data=exp_data)
    assert loader.flip and not valid.flip                                     # the training loader only
    seen = []
    for batch, metas in loader:
        flips = (loader.last["draws"] <= 0.5).cpu().tolist()
        seen += flips
        rows = [m["image_id"] - 100 for m in metas]
        want1 = np.stack([R.stage1(images[k], 48, f) for k, f in zip(rows, flips)])
        assert np.array_equal(batch.stage1.cpu().numpy(), want1) and torch.equal(batch.canvas.cpu(), _preprocess(want1, 64))
        new_w, new_h = E.resize_meta(48, 48, 64)[:2]
        gt, _ = R.gt_table([L_BOXES[k] for k in rows], [L_LABELS[k] for k in rows], [L_SIZES[k] for k in rows], 48, new_w / 48, new_h / 48, flips)
        assert np.array_equal(batch.gt.cpu().numpy(), gt)
    assert len(seen) == 4


def test_loader_and_loss_do_not_wait_for_the_device(trainable):
    loader, _, _ = _loader(True, canvas_size=E.MAX_SIZE)
    warm = next(iter(loader))[0]
    out = trainable.detection_loss(warm)                                      # builds the plan, the training buffers and the record-free path
    (out["classification"] + out["regression"]).backward()
    torch.cuda.synchronize()
    loader.set_epoch(0)
    it = iter(loader)                                                         # the epoch's indices go up here, before the first batch
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [b for b, _ in it]                                          # a whole epoch of the loader
        out = trainable.detection_loss(batches[0])                            # up to and including the returned loss tensors
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(batches) == 2 and torch.isfinite(out["classification"]) and torch.isfinite(out["regression"])
    (out["classification"] + out["regression"]).backward()


# ------------------------------------------------------------------------------------------------ DetectorTrainer
T_SIZES = [(96, 128), (120, 90), (100, 100), (80, 110)]
T_BOXES = [np.array([[10, 12, 70, 80], [60, 20, 120, 60]], np.float32), np.array([[5, 10, 80, 110]], np.float32),
           np.array([[20, 20, 90, 90]], np.float32), np.array([[8, 8, 100, 70], [30, 10, 60, 40]], np.float32)]
T_LABELS = [[1, 1], [1], [1], [1, 1]]


def _exp_data():
    return {"training": {"num_epochs": 2, "save_frequency": 1, "learning_rate": 1e-3, "learning_rate_factor": 0.5, "patience": 1,
                         "momentum": 0.9, "optimizer": "adam", "nesterov": False, "scheduler": "plateau", "perceptual_loss": False},
            "dataset": {"dataset_name": "coco", "image_size": 256}}


def _trainer(exp_path, store, db, **kw):
    model = _model(train_header=True)
    exp = _exp_data()
    train = DetBatchLoader(db, store, exp, 2, True, seed=3)
    valid = DetBatchLoader(db, store, exp, 2, False)
    assert train.image_size == valid.image_size == 256
    return DetectorTrainer(str(exp_path), exp, model, train, valid, db.coco_gt(256), valid_fraction=1.0, **kw)


def test_detector_evaluator_takes_the_loader_in_both_output_modes(detector):
    from stlpose_amd.detection_eval import CocoEvaluator, DetectorEvaluator
    images = DR.images() + [np.ascontiguousarray(im[::-1]) for im in DR.images()]   # the detector's fixture images: they have detections
    db = _db([im.shape[:2] for im in images], T_BOXES, T_LABELS)
    store = ResidentImages.from_arrays(images, DEV)
    valid = DetBatchLoader(db, store, None, 3, False, image_size=400)         # batches of 3 and 1
    gt = db.coco_gt(400)
    host = DetectorEvaluator(detector, output="host")
    device = DetectorEvaluator(detector, output="device")
    a, b = host.evaluate(valid, gt), device.evaluate(valid, gt)
    assert np.array_equal(a["stats"], b["stats"]) and a["valid_ap"] == b["valid_ap"]
    assert host.coco_evaluator.img_ids == device.coco_evaluator.img_ids == [100, 101, 102, 103]
    # the same detections, fed by hand
    ev = CocoEvaluator(gt, ("bbox",))
    n = 0
    for batch, metas in valid:
        outs = detector(batch)
        n += sum(len(o["scores"]) for o in outs)
        ev.update({m["image_id"]: o for m, o in zip(metas, outs)})
    assert n > 0
    assert np.array_equal(ev.summarize()["bbox"], a["stats"])
    fifth = device.evaluate(DetBatchLoader(db, store, None, 1, False, image_size=400), gt, fraction=0.5)   # the first two batches
    assert device.coco_evaluator.img_ids == [100, 101] and len(fifth["stats"]) == 12


def test_detector_trainer_trains_saves_and_resumes(tmp_path):
    images, db = _images(T_SIZES, 21), _db(T_SIZES, T_BOXES, T_LABELS)
    store = ResidentImages.from_arrays(images, DEV)
    t = _trainer(tmp_path / "full", store, db)
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    t.training_loop()
    logs = json.loads((tmp_path / "full" / "detector_logs.json").read_text())
    print("trainer logs", logs, "skipped", t.skipped)
    assert len(logs["train_loss"]) == 2 and len(logs["valid_ap"]) == 2 and all(np.isfinite(logs["train_loss"])) and t.skipped == 0
    heads = {n for n, _ in head_parameters(t.model)}
    after = t.model.state_dict()
    moved = {k for k in heads if not torch.equal(after[k], before[k])}
    # every classifier parameter has a gradient (each anchor is a negative at least); the regressor's come from the positive
    # anchors alone, so a level without one leaves its own BN parameters where they were: the shared ones must have moved
    assert {k for k in heads if k.startswith("classifier.")} <= moved
    assert {k for k in heads if k.startswith("regressor.") and ".bn_list." not in k} <= moved
    assert any(k.startswith("regressor.bn_list.") for k in moved)
    for k, v in after.items():
        if not (k.startswith("regressor.") or k.startswith("classifier.")):   # the backbone and the BiFPN, buffers included
            assert torch.equal(v, before[k]), k
    saved = tmp_path / "full" / "models" / "detector"
    assert sorted(os.listdir(saved)) == ["checkpoint_epoch_0.pth", "checkpoint_epoch_1.pth", "checkpoint_epoch_final.pth"]
    ck = torch.load(saved / "checkpoint_epoch_final.pth", weights_only=False)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"] and ck["epoch"] == 2
    # the final checkpoint in a fresh model: the trained model's outputs, exactly
    fresh = E.setup_detector("efficientdet", "d0")
    fresh.load_state_dict(ck["model_state_dict"], strict=True)
    fresh = fresh.to(DEV)
    batch, _ = t.valid_loader[0]
    _same_list(fresh(batch), t.model(batch))
    _same_list(fresh(batch, output="device").to_list(), t.model(batch))
    got, want = fresh(batch, postprocess=False), t.model(batch, postprocess=False)
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    # resumed behind the first epoch: the weights of the uninterrupted run
    os.makedirs(tmp_path / "resumed")
    shutil.copy(tmp_path / "full" / "detector_logs.json", tmp_path / "resumed" / "detector_logs.json")
    r = _trainer(tmp_path / "resumed", store, db, checkpoint=str(saved / "checkpoint_epoch_0.pth"), resume_training=True)
    assert r.cur_epoch == 1
    r.training_loop()
    for k, v in after.items():
        assert torch.equal(v, r.model.state_dict()[k]), k
