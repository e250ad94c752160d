"""GPU: top-down extraction kernels (csrc/topdown.hip) against the restatements in tests/topdown_ref.py, torch on the device and
the reference's own outputs (tests/golden/topdown/g14_topdown.npz), and PoseExtractor / extract_retrieval_db end to end."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stlpose_amd  # noqa: F401,E402  (registers the stlpose:: ops)
from tests import topdown_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "topdown", "g14_topdown.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(FIX)


# ------------------------------------------------------------------------------------------------ 1. box_select vs restatement
def _ragged(rng, sizes):
    boxes, scores = [], []
    for n in sizes:
        xy = rng.uniform(0, 1000, (n, 2))
        b = np.concatenate([xy, xy + rng.uniform(2, 150, (n, 2))], 1).astype(np.float32)
        s = rng.choice(np.linspace(0.05, 1, 40), n).astype(np.float32)   # many exact ties
        if n >= 8:
            d = rng.choice(n, n // 8, replace=False)
            b[d] = b[(d + 1) % n]                                         # duplicates
            b[d[: len(d) // 2], 2] = b[d[: len(d) // 2], 0]               # zero width
        boxes.append(b), scores.append(s)
    return boxes, scores


def test_box_select_matches_restatement():
    rng = np.random.default_rng(5)
    sizes = [0, 1, 63, 64, 65, 1000, 4096]
    boxes, scores = _ragged(rng, sizes)
    b, s = torch.from_numpy(np.concatenate(boxes)).cuda(), torch.from_numpy(np.concatenate(scores)).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    for thr in (0.3, 0.5, 0.7):
        keep, count = torch.ops.stlpose.box_select(b, s, None, off, 1, None, thr)
        keep, count = keep.cpu().numpy(), count.cpu().numpy()
        for i, n in enumerate(sizes):
            want = R.nms(boxes[i], scores[i], thr)
            seg = keep[off[i]:off[i + 1]]
            assert count[i] == len(want), (thr, n)
            assert np.array_equal(seg[:count[i]], want), (thr, n)
            assert (seg[count[i]:] == -1).all()
    # filter only: label and score test, input order kept
    lab = torch.from_numpy(rng.integers(1, 3, len(s))).cuda()
    keep, count = torch.ops.stlpose.box_select(b, s, lab, off, 1, 0.5, -1.0)
    keep, count, labh, sh = keep.cpu().numpy(), count.cpu().numpy(), lab.cpu().numpy(), s.cpu().numpy()
    for i in range(len(sizes)):
        want = np.nonzero((labh[off[i]:off[i + 1]] == 1) & (sh[off[i]:off[i + 1]] > np.float32(0.5)))[0]
        assert count[i] == len(want) and np.array_equal(keep[off[i]:off[i] + count[i]], want)


def test_box_select_refuses_over_cap():
    b = torch.zeros(4097, 4, device="cuda")
    with pytest.raises(ValueError, match="4096"):
        torch.ops.stlpose.box_select(b, torch.zeros(4097, device="cuda"), None, torch.tensor([0, 4097]), 1, None, 0.5)


# ------------------------------------------------------------------------------------------------ 2. drop-ins vs G14
def test_bbox_filtering_and_nms_match_reference(g):
    from stlpose_amd import bbox_filtering, bbox_nms
    off = g["det_offsets"]
    preds = [{"boxes": torch.from_numpy(g["det_boxes"][a:b]).cuda(), "labels": torch.from_numpy(g["det_labels"][a:b]).cuda(),
              "scores": torch.from_numpy(g["det_scores"][a:b]).cuda()} for a, b in zip(off[:-1], off[1:])]
    fb, fl, fs = bbox_filtering(preds, filter_=1, thr=0.6)
    assert [len(x) for x in fb] == list(g["filt_count"])
    assert np.array_equal(np.concatenate(fb), g["filt_boxes"]) and np.array_equal(np.concatenate(fl), g["filt_labels"])
    assert np.array_equal(np.concatenate(fs), g["filt_scores"])
    nb, nl, ns = bbox_nms(fb, fl, fs, nms_thr=0.5)
    assert [len(x) for x in nb] == list(g["nms_filt_count"])
    assert np.array_equal(np.concatenate(nb), g["nms_filt_boxes"]) and np.array_equal(np.concatenate(nl), g["nms_filt_labels"])
    assert np.array_equal(np.concatenate(ns), g["nms_filt_scores"])
    assert nb[0].shape == (0, 4) and nl[0].shape == (0,)
    for t in (0.3, 0.5, 0.7):
        raw_b = [g["det_boxes"][a:b] for a, b in zip(off[:-1], off[1:])]
        raw_s = [g["det_scores"][a:b] for a, b in zip(off[:-1], off[1:])]
        rows = [np.arange(b - a) for a, b in zip(off[:-1], off[1:])]
        _, kl, _ = bbox_nms(raw_b, rows, raw_s, nms_thr=t)
        assert [len(x) for x in kl] == list(g[f"nms_raw_{t}_count"])
        assert np.array_equal(np.concatenate(kl), g[f"nms_raw_{t}_idx"])


# ------------------------------------------------------------------------------------------------ 3. fused decode
def _ulp(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


def _check_decode(hm, ho, wo):
    idx, mx, preds = torch.ops.stlpose.heatmap_resize_argmax(hm, ho, wo)
    up = F.interpolate(hm, (ho, wo), mode="bilinear", align_corners=True)
    tidx, tmx, _ = torch.ops.stlpose.heatmap_argmax(up)
    t = up.reshape(hm.shape[0], hm.shape[1], -1).cpu().numpy().astype(np.float64)
    idx, mx, preds = idx.cpu().numpy(), mx.cpu().numpy(), preds.cpu().numpy()
    tidx, tmx = tidx.cpu().numpy(), tmx.cpu().numpy()[..., 0]
    for b in range(hm.shape[0]):
        for j in range(hm.shape[1]):
            row, m = t[b, j], tmx[b, j]
            if np.isnan(m):
                assert np.isnan(mx[b, j]) and idx[b, j] == tidx[b, j]
                continue
            u = _ulp(m)
            assert row[idx[b, j]] >= m - 4 * u, (b, j)
            second = np.max(np.delete(row, tidx[b, j])) if row.size > 1 else -np.inf
            if m - second > 4 * u:
                assert idx[b, j] == tidx[b, j], (b, j)
            assert abs(float(mx[b, j]) - m) <= 2 * u, (b, j)
            gate = 1.0 if mx[b, j] > 0 else 0.0
            assert preds[b, j, 0] == (idx[b, j] % wo) * gate and preds[b, j, 1] == (idx[b, j] // wo) * gate
    return idx, mx, preds


def test_heatmap_resize_argmax_against_torch():
    gen = torch.Generator(device="cuda").manual_seed(11)
    for (h, w, ho, wo) in ((64, 48, 256, 192), (96, 72, 384, 288), (64, 48, 64, 48)):
        hm = torch.rand(37, 17, h, w, device="cuda", generator=gen)
        hm[3, 2, 10, 7] = float("nan")
        hm[4, 3, 20, 5] = float("-inf")
        hm[5, 4] = -hm[5, 4] - 0.1
        hm[6, 1] = 0.25
        idx, mx, preds = _check_decode(hm, ho, wo)
        assert np.isnan(mx[3, 2])
        assert mx[5, 4] < 0 and (preds[5, 4] == 0).all()
        assert idx[6, 1] == 0 and mx[6, 1] == np.float32(0.25)
        # the kernel is the float32 restatement exactly
        x = hm[:4].cpu().numpy()
        r = R.resize_bilinear(x, ho, wo).reshape(4, 17, -1)
        want = R.argmax_first(r)
        assert np.array_equal(idx[:4], want)
        assert np.array_equal(mx[:4], np.take_along_axis(r, want[..., None], -1)[..., 0], equal_nan=True)


def test_create_pose_from_outputs_matches_reference(g):
    from stlpose_amd import create_pose_from_outputs
    entries, all_kp = create_pose_from_outputs(torch.from_numpy(g["hm"]).cuda(), keypoint_thr=0.1)
    assert np.array_equal(np.stack(entries), g["cpo_entries"])
    assert all_kp.dtype == g["cpo_all"].dtype and np.array_equal(all_kp, g["cpo_all"])


# ------------------------------------------------------------------------------------------------ 4. TransformDetection
def test_transform_detection_matches_reference_and_crop_batch(g):
    from stlpose_amd import TransformDetection
    from stlpose_amd.augment import crop_batch
    rng = np.random.default_rng(8)
    img = torch.from_numpy(rng.integers(0, 256, (480, 560, 3), dtype=np.uint8))
    t = TransformDetection(det_width=192, det_height=256)
    dets, c, s = t(img, g["td_coords"])
    assert np.array_equal(c, g["td_centers"]) and np.array_equal(s, g["td_scales"])
    assert dets.is_cuda and tuple(dets.shape) == (len(c), 3, 256, 192)
    n = len(c)
    box = (s * np.float32(200)).astype(np.float64) / 200.0
    want, trans = crop_batch([img.cuda()] * n, c, box, np.zeros(n), np.zeros(n, bool), (192, 256))
    assert np.array_equal(trans, g["td_trans"])
    assert torch.equal(dets, want)
    empty, ce, se = t(img, np.zeros((0, 4), np.float32))
    assert empty.shape[0] == 0 and ce.shape == (0, 2)


# ------------------------------------------------------------------------------------------------ 5. PoseExtractor
def _load_synth(model):
    from oracle import hrnet_ref
    sd = {k: torch.from_numpy(hrnet_ref.synth_tensor(k, tuple(v.shape))) for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    return model


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(21)
    images = [torch.from_numpy(rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)) for hw in ((200, 240), (320, 300), (360, 420))]
    boxes, scores = [], []
    for n, (h, w) in zip((0, 5, 41), ((200, 240), (320, 300), (360, 420))):
        xy = rng.uniform(0, min(h, w) * 0.6, (n, 2))
        b = np.concatenate([xy, xy + rng.uniform(20, 120, (n, 2))], 1).astype(np.float32)
        s = rng.uniform(0.75, 1.0, n).astype(np.float32)
        if n:
            b[n - 1] = b[0]                      # a duplicate NMS removes
            s[n - 1] = s[0] * np.float32(0.99)
        boxes.append(b), scores.append(s)
    return images, boxes, scores


def _by_hand(model, images, boxes, scores, batch, flip):
    """bbox_nms -> TransformDetection -> the model on the same padded chunks -> final_preds."""
    from stlpose_amd import TransformDetection, bbox_nms, forward_pass
    nb, _, _ = bbox_nms(boxes, [np.ones(len(b), np.int64) for b in boxes], scores, nms_thr=0.5)
    t = TransformDetection()
    crops, cs, ss = [], [], []
    for im, b in zip(images, nb):
        if len(b):
            d, c, s = t(im, b)
            crops.append(d), cs.append(c), ss.append(s)
    x = torch.cat(crops)
    outs = []
    for a in range(0, x.shape[0], batch):
        ch = x[a:a + batch]
        n = ch.shape[0]
        ch = torch.cat([ch, ch.new_zeros(batch - n, *ch.shape[1:])])
        with torch.no_grad():
            outs.append(forward_pass(model, ch, flip=flip)[:n])
    hm = torch.cat(outs)
    p, m = torch.ops.stlpose.final_preds(hm, torch.from_numpy(np.concatenate(cs)).cuda(), torch.from_numpy(np.concatenate(ss)).cuda())
    return nb, torch.cat([p, m], 2).cpu().numpy()


@pytest.mark.parametrize("flip", [False, True])
def test_pose_extractor_end_to_end(scene, flip):
    from stlpose_amd import PoseExtractor, PoseHighResolutionNet
    model = _load_synth(PoseHighResolutionNet("tiny", "fp32")).cuda().eval()
    images, boxes, scores = scene
    ex = PoseExtractor(model, flip=flip, batch=8)
    res = ex(images, boxes, scores, det_thr=0.7, nms_thr=0.5)
    assert len(model._engines) == 1 and next(iter(model._engines))[0] == 8
    nb, kp = _by_hand(model, images, boxes, scores, 8, flip)
    assert len(model._engines) == 1
    assert [len(r["boxes"]) for r in res] == [len(b) for b in nb] and len(nb[2]) < 41
    got = np.concatenate([r["keypoints"] for r in res])
    assert got.dtype == np.float32 and np.array_equal(got, kp)
    assert res[0]["keypoints"].shape == (0, 17, 3) and res[0]["pose_entries"] == []
    for r in res[1:]:
        n = len(r["boxes"])
        assert r["crop_keypoints"].shape == (n, 17, 3) and r["all_keypoints"].shape == (n * 17, 4) and len(r["pose_entries"]) == n
        assert np.array_equal(r["all_keypoints"][:, 1], np.where((r["keypoints"][..., :2] == -1).any(-1), -1,
                                                                  r["keypoints"][..., 0]).reshape(-1))
    # the same person in a full chunk and in a padded one: the third image alone shifts every person by the second's count
    alone = ex(images[2:], boxes[2:], scores[2:], det_thr=0.7, nms_thr=0.5)[0]
    assert np.array_equal(alone["keypoints"], res[2]["keypoints"]) and np.array_equal(alone["crop_keypoints"], res[2]["crop_keypoints"])
    assert len(model._engines) == 1


# ------------------------------------------------------------------------------------------------ 6. retrieval database
class _TableModel:
    """Stands in for the network: returns the fixture's heat map of the image whose corner pixel names it."""
    training = False

    def __init__(self, hm):
        self.hm = torch.from_numpy(hm).cuda()

    def __call__(self, x):
        return self.hm[x[:, 0, 0, 0].long()]


def test_extract_retrieval_db_round_trip(g, tmp_path):
    from stlpose_amd import (PoseHighResolutionNet, extract_retrieval_db, fit_knn_structure, load_knn, process_pose_vectors)
    n = g["hm"].shape[0]
    imgs = torch.zeros(n, 3, 256, 192)
    imgs[:, 0, 0, 0] = torch.arange(n, dtype=torch.float32)
    loader = [(imgs[i:i + 1], None, None, {"center": torch.tensor([[96.0 + i, 128.0]]), "scale": torch.tensor([[1.0, 1.33]]),
                                            "image": [f"vase_{i}.png"], "character_name": [f"char_{i % 2}"]}) for i in range(n)]
    db = extract_retrieval_db(_TableModel(g["hm"]), loader, flip=False)
    assert list(db) == [f"img_{i}" for i in range(n)]
    for i in range(n):
        e = db[f"img_{i}"]
        assert e["img"] == f"vase_{i}.png" and e["character_name"] == f"char_{i % 2}"
        assert e["joints"].dtype == torch.float32 and torch.equal(e["joints"], torch.from_numpy(g["rdb_joints"][i]))
        assert tuple(e["center"].shape) == (1, 2) and float(e["center"][0, 0]) == 96.0 + i
    # the real network with the flip test, then the retrieval index written and read back
    model = _load_synth(PoseHighResolutionNet("tiny", "fp32")).cuda().eval()
    rng = np.random.default_rng(2)
    real = [(torch.from_numpy(rng.normal(size=(1, 3, 256, 192)).astype(np.float32)), None, None,
             {"center": torch.tensor([[96.0, 128.0]]), "scale": torch.tensor([[1.0, 1.33]]), "image": [f"r{i}"],
              "character_name": ["c"]}) for i in range(3)]
    db = extract_retrieval_db(model, real, flip=True)
    joints = torch.stack([db[k]["joints"] for k in db])
    vec = process_pose_vectors(joints, "full_body", True)
    params = types.SimpleNamespace(database_file="db_topdown.pkl", metric="euclidean_distance", approach="full_body", normalize=True)
    name = fit_knn_structure(vec, db, params, str(tmp_path))
    knn, database, features = load_knn(f"data_{name}", str(tmp_path))
    assert np.array_equal(features, vec.cpu().numpy()) and list(database) == list(db)
    idx, _ = knn.knn_query(vec.cpu().numpy(), k=1)
    assert np.array_equal(features[np.asarray(idx).reshape(-1).astype(np.int64)], features)
