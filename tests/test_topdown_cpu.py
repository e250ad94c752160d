"""CPU: the host half of top-down extraction against fixture G14 (the reference's own lib/bounding_box.py, lib/pose_parsing.py
and lib/transforms.py outputs), the restatements in tests/topdown_ref.py, and the argument checks made before any launch."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import topdown_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "topdown", "g14_topdown.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(FIX)


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference tree exists in the build container only")
def test_topdown_generator_reproduces_fixture(tmp_path):
    env = dict(os.environ, STL_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "topdown", "make_golden_topdown.py")], check=True,
                   env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=600)
    a, b = np.load(FIX), np.load(os.path.join(str(tmp_path), "g14_topdown.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    assert not glob.glob("/root/reference/**/__pycache__", recursive=True)


def test_fixture_layout(g):
    assert os.path.getsize(FIX) < 1 << 20
    assert list(np.diff(g["det_offsets"])) == [0, 1, 9, 40, 120]
    assert g["hm"].shape == (4, 17, 64, 48) and (g["hm"][2, 5] < 0).all() and (g["hm"][3, 7] == g["hm"][3, 7, 0, 0]).all()
    assert (g["ce_all"][:, 0] == -1).sum() == 3


def test_create_pose_entries_matches_reference(g):
    from stlpose_amd import create_pose_entries
    entries, all_kp = create_pose_entries(g["ce_keypoints"], g["ce_maxvals"], thr=0.1)
    assert all_kp.dtype == g["ce_all"].dtype and np.array_equal(all_kp, g["ce_all"])
    assert len(entries) == 3 and all(e.shape == (19,) for e in entries)
    assert np.array_equal(np.stack(entries), g["ce_entries"])
    e2, a2 = create_pose_entries(g["ce_keypoints"].astype(np.int64))   # int input keeps int rows, no thresholding
    assert a2.dtype == np.int64 and (a2[:, 3] != 0).all()
    assert create_pose_entries([]) == ([], [])


def test_bbox_to_image_keypoints_matches_reference(g):
    from stlpose_amd import bbox_to_image_keypoints
    boxes = [g["bk_boxes"][:1], np.zeros((0, 4), np.float32), g["bk_boxes"][1:]]
    out = bbox_to_image_keypoints(g["bk_pred"].copy(), boxes, height=256, width=192)
    assert out.dtype == g["bk_out"].dtype and np.array_equal(out, g["bk_out"])
    same = g["bk_pred"].copy()
    assert bbox_to_image_keypoints(same, [[], []]) is same


def test_coords2cs_and_matrices_match_reference(g):
    from stlpose_amd import TransformDetection
    t = TransformDetection(det_width=192, det_height=256)
    c, s = t.coords2cs(g["td_coords"])
    assert c.dtype == s.dtype == np.float32
    assert np.array_equal(c, g["td_centers"]) and np.array_equal(s, g["td_scales"])
    for i in range(len(c)):
        ci, si = t._coords2cs(list(g["td_coords"][i]))
        assert np.array_equal(ci, g["td_centers"][i]) and np.array_equal(si, g["td_scales"][i])
    assert np.array_equal(t.matrices(c, s), g["td_trans"])


def test_get_detections_matches_reference(g):
    from stlpose_amd import get_detections
    b = g["gd_boxes"]
    crops = get_detections(torch.from_numpy(g["gd_imgs"]), [[b[0], b[1]], [b[2], b[3]]], height=32, width=24)
    assert np.array_equal(crops.numpy(), g["gd_crops"])
    assert get_detections(torch.from_numpy(g["gd_imgs"]), [[], []]) == []


def test_nms_restatement_on_fixture(g):
    """The restatement the generator used for torchvision.ops.nms, re-run: per-image kept rows as stored."""
    off = g["det_offsets"]
    for t in (0.3, 0.5, 0.7):
        idx, cnt = g[f"nms_raw_{t}_idx"], g[f"nms_raw_{t}_count"]
        pos = 0
        for i, (a, b) in enumerate(zip(off[:-1], off[1:])):
            k = R.nms(g["det_boxes"][a:b], g["det_scores"][a:b], t)
            assert len(k) == cnt[i] and np.array_equal(k, idx[pos:pos + cnt[i]])
            pos += cnt[i]


def test_nms_restatement_semantics():
    b = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [1, 1, 9, 9], [20, 20, 20, 30], [20, 20, 20, 30], [50, 50, 60, 60]], np.float32)
    s = np.array([0.5, 0.5, 0.9, 0.7, 0.7, 0.1], np.float32)
    # 2 first (highest), it contains 0 and 1 (IoU 0.64 each); zero-area boxes never suppress each other (0 / 0)
    assert list(R.nms(b, s, 0.5)) == [2, 3, 4, 5]
    assert list(R.nms(b, s, 0.7)) == [2, 3, 4, 0, 5]   # the tie 0 / 1 goes to the lower index, 1 is its duplicate
    assert len(R.nms(np.zeros((0, 4)), np.zeros(0), 0.5)) == 0


def test_resize_restatement_against_torch():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(2, 3, 16, 12)).astype(np.float32)
    for ho, wo in ((64, 48), (16, 12), (33, 7), (1, 5)):
        want = F.interpolate(torch.from_numpy(x), (ho, wo), mode="bilinear", align_corners=True).numpy()
        np.testing.assert_allclose(R.resize_bilinear(x, ho, wo), want, rtol=0, atol=2e-6)


def test_wrappers_refuse_before_launch():
    from stlpose_amd import ops
    b = torch.zeros(4097, 4)
    with pytest.raises(ValueError, match="4096"):
        ops._box_select(b, torch.zeros(4097), None, torch.tensor([0, 4097]), 1, None, 0.5)
    with pytest.raises(ValueError, match="float32"):
        ops._box_select(b.double(), torch.zeros(4097), None, torch.tensor([0, 4097]), 1, None, 0.5)
    with pytest.raises(ValueError, match="16384"):
        ops._resize_argmax(torch.zeros(1, 1, 129, 128), 256, 192)
    with pytest.raises(ValueError, match="float32"):
        ops._resize_argmax(torch.zeros(1, 1, 64, 48, dtype=torch.float16), 256, 192)
