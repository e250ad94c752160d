"""CPU: the EfficientDet detector's state_dict layout, anchors, preprocess sizes and setup_detector against the reference's own
outputs (tests/golden/detector/g15_effdet.npz), and the restatements of tests/detector_ref.py (eager network, postprocess with
torchvision 0.4's batched_nms) against the same fixture."""
import os

import numpy as np
import pytest
import torch

from stlpose_amd import efficientdet as E
from tests import detector_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "detector", "g15_effdet.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(FIX)


def _layout(g, cc):
    rows = bytes(g[f"d{cc}_layout"]).decode().split("\n")
    return {k: tuple(int(v) for v in s.split(",") if v) for k, s in (r.split(" ") for r in rows)}


@pytest.mark.parametrize("cc", [0, 3])
def test_state_dict_layout_and_strict_load(g, cc):
    ref = _layout(g, cc)
    m = E.EfficientDetBackbone(num_classes=1, compound_coef=cc)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(mine) == list(ref)
    assert mine == ref
    sd = R.synth_state_dict(ref)
    m.load_state_dict(sd, strict=True)
    m.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)   # a DataParallel save
    assert torch.equal(m.state_dict()["backbone_net.model._blocks.3._depthwise_conv.conv.weight"],
                       sd["backbone_net.model._blocks.3._depthwise_conv.conv.weight"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in list(sd.items())[1:]}, strict=True)


def test_anchors_and_metas(g):
    a = torch.from_numpy(E.anchors(0)).double()[None]
    assert a.shape == (1, 49104, 4)
    s = np.array([a.sum().item(), (a * torch.arange(a.shape[1])[None, :, None]).sum().item()])
    np.testing.assert_array_equal(s, g["anchors_sum"])
    metas = [E.resize_meta(*im.shape[:2]) for im in R.images()]
    np.testing.assert_array_equal(np.array(metas, np.int64), g["metas"])


def test_preprocess_restatement(g):
    for i, im in enumerate(R.images()):
        x = (im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - np.array(E.MEAN, np.float32)[:, None, None]) \
            / np.array(E.STD, np.float32)[:, None, None]
        nw, nh = E.resize_meta(*im.shape[:2])[:2]
        canvas = np.zeros((512, 512, 3), np.float32)
        canvas[:nh, :nw] = R.resize_linear(x.transpose(1, 2, 0), nw, nh)
        np.testing.assert_allclose(canvas.transpose(2, 0, 1)[:, ::8, ::8], g["canvas_s"][i], rtol=0, atol=1e-5)


def test_eager_restatement_matches_reference(g):
    sd = R.synth_state_dict(_layout(g, 0))
    ims = R.images()
    canvas = np.zeros((2, 3, 512, 512), np.float32)
    for i, im in enumerate(ims):
        x = (im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - np.array(E.MEAN, np.float32)[:, None, None]) \
            / np.array(E.STD, np.float32)[:, None, None]
        nw, nh = E.resize_meta(*im.shape[:2])[:2]
        canvas[i, :, :nh, :nw] = R.resize_linear(x.transpose(1, 2, 0), nw, nh).transpose(2, 0, 1)
    with torch.no_grad():
        feats, reg, cls = R.eager_forward(sd, 0, 1, torch.from_numpy(canvas))
    for i, f in enumerate(feats):
        ref = g[f"f{i}_s"]
        np.testing.assert_allclose(f[:, ::4, ::4, ::4].numpy(), ref, rtol=0, atol=1e-4 * np.abs(ref).max())
    np.testing.assert_allclose(cls.numpy(), g["cls"], rtol=0, atol=1e-4)
    for i in range(2):
        ref = g[f"cand{i}_reg"]
        np.testing.assert_allclose(reg[i, g[f"cand{i}_idx"]].numpy(), ref, rtol=0, atol=1e-4 * np.abs(ref).max())


def ref_heads(g):
    """The reference's own head outputs for every anchor the postprocess reads: the full classification and the regression
    rows of the anchors above lo_thr (the other rows never pass either threshold and stay 0)."""
    reg = np.zeros((2, 49104, 4), np.float32)
    for i in range(2):
        reg[i, g[f"cand{i}_idx"]] = g[f"cand{i}_reg"]
    return reg, g["cls"]


def check_detections(g, dets, metas):
    """dets: per image (boxes on the canvas, classes, scores) at threshold 0.5 -> the reference's forward dicts exactly."""
    for i, (b, c, s) in enumerate(dets):
        np.testing.assert_array_equal(s, g[f"det{i}_scores"])
        np.testing.assert_array_equal(c.astype(np.int32) + 1, g[f"det{i}_labels"])
        np.testing.assert_allclose(E.invert_affine(metas[i], b), g[f"det{i}_boxes"], rtol=0, atol=1e-4)


def check_low(g, dets):
    """dets at threshold lo_thr (> 4096 candidates in image 0) -> the reference's postprocess exactly, on the canvas."""
    for i, (b, c, s) in enumerate(dets):
        np.testing.assert_array_equal(s, g[f"lo{i}_scores"])
        np.testing.assert_array_equal(c, g[f"lo{i}_class_ids"])
        np.testing.assert_allclose(b, g[f"lo{i}_rois"], rtol=0, atol=1e-4)


def test_postprocess_restatement_matches_reference(g):
    """detector_ref's decode + batched_nms on the reference's own head outputs reproduces its detections exactly: the forward's
    dicts at threshold 0.5 (after invert_affine) and the postprocess at lo_thr, > 4096 candidates in one image."""
    reg, cls = ref_heads(g)
    a = E.anchors(0)
    metas = [tuple(int(v) for v in m) for m in g["metas"]]
    check_detections(g, R.postprocess(a, reg, cls, 0.5, 0.5), metas)
    assert int((cls[0].max(1) > g["lo_thr"]).sum()) > 4096
    check_low(g, R.postprocess(a, reg, cls, float(g["lo_thr"]), 0.5))


def test_setup_detector():
    m = E.setup_detector("efficientdet", "d0")
    assert isinstance(m, E.EfficientDet) and m.compound_coef == 0 and m.num_classes == 1
    assert m.threshold == 0.5 and m.iou_threshold == 0.5
    assert E.setup_detector("efficientdet", "d3").compound_coef == 3
    with pytest.raises(NotImplementedError, match="torchvision"):
        E.setup_detector("faster_rcnn")
    with pytest.raises(ValueError):
        E.setup_detector("yolo")
    with pytest.raises(ValueError):
        E.setup_detector("efficientdet", "d7")
    with pytest.raises(NotImplementedError):
        E.EfficientDetBackbone(compound_coef=1)
    with pytest.raises(NotImplementedError):
        E.EfficientDetBackbone(load_weights=True)
    m.train()
    with pytest.raises(NotImplementedError, match="inference"):
        m(torch.zeros(1, 3, 64, 64))
