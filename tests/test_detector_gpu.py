"""GPU: the EfficientDet kernels (csrc/detector.hip) against torch restatements on the device, and the detector end to end
against the reference's own outputs (tests/golden/detector/g15_effdet.npz) and tests/detector_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import capi, efficientdet as E
from tests import detector_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "detector", "g15_effdet.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def g():
    return np.load(FIX)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _layout(g, cc):
    rows = bytes(g[f"d{cc}_layout"]).decode().split("\n")
    return {k: tuple(int(v) for v in s.split(",") if v) for k, s in (r.split(" ") for r in rows)}


def _close(a, b, rel=1e-3):
    a, b = a.float().cpu(), torch.as_tensor(b).float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= rel * max(b.abs().max().item(), 1e-6), (err, b.abs().max().item())


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("hw", [(17, 12), (16, 9)])
def test_dwconv_same_padding(k, s, hw):
    torch.manual_seed(k * 10 + s)
    B, C = 2, 24
    x = torch.randn(B, C, *hw, device=DEV)
    w = torch.randn(C, 1, k, k, device=DEV)
    bias = torch.randn(C, device=DEV)
    ref = F.silu(F.conv2d(R._same(x, k, s), w, bias, s, 0, 1, C))
    xn = x.permute(0, 2, 3, 1).contiguous()
    wk = w[:, 0].permute(1, 2, 0).contiguous()
    out = torch.empty(B, ref.shape[2], ref.shape[3], C, device=DEV)
    capi.call("stl_det_dwconv", xn.data_ptr(), wk.data_ptr(), bias.data_ptr(), out.data_ptr(), B, hw[0], hw[1], C, k, s, 1, _st())
    _close(out.permute(0, 3, 1, 2), ref, 1e-5)


@pytest.mark.parametrize("hw", [(17, 12), (16, 9)])
def test_stem_same_padding(hw):
    torch.manual_seed(hw[1])
    B, Co = 2, 40
    x = torch.randn(B, 3, *hw, device=DEV)
    w = torch.randn(Co, 3, 3, 3, device=DEV)
    bias = torch.randn(Co, device=DEV)
    ref = F.silu(F.conv2d(R._same(x, 3, 2), w, bias, 2))
    xn = x.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(B, ref.shape[2], ref.shape[3], Co, device=DEV)
    capi.call("stl_det_stem", xn.data_ptr(), w.permute(2, 3, 1, 0).contiguous().data_ptr(), bias.data_ptr(), out.data_ptr(), B, hw[0],
              hw[1], Co, _st())
    _close(out.permute(0, 3, 1, 2), ref, 1e-5)


def _pointwise(x, w, bias, act, in_scale=None, residual=None):
    B, H, W, ci = x.shape
    co = w.shape[0]
    kp, np_ = -(-ci // 16) * 16, -(-co // 64) * 64
    wp = torch.zeros(kp, np_, device=DEV)
    wp[:ci, :co] = w.t()
    bp = torch.zeros(np_, device=DEV)
    bp[:co] = bias
    out = torch.empty(B, H, W, co, device=DEV)
    p = capi.DetPointwise(x.data_ptr(), wp.data_ptr(), bp.data_ptr(), None if in_scale is None else in_scale.data_ptr(),
                          None if residual is None else residual.data_ptr(), out.data_ptr(), B * H * W, H * W * co, co, 0, H * W, ci,
                          co, kp, np_, act)
    capi.call("stl_det_pointwise", C.byref(p), _st())
    return out


@pytest.mark.parametrize("ci,co", [(6, 9), (37, 36), (1152, 1392 // 4), (13, 1)])
def test_pointwise_se_residual(ci, co):
    torch.manual_seed(ci)
    B, H, W = 2, 7, 9
    x = torch.randn(B, H, W, ci, device=DEV)
    w = torch.randn(co, ci, device=DEV) / ci ** 0.5
    bias = torch.randn(co, device=DEV)
    sc = torch.rand(B, ci, device=DEV)
    res = torch.randn(B, H, W, co, device=DEV)
    xs = x * sc[:, None, None, :]
    ref = F.silu(xs.double() @ w.t().double() + bias.double()) + res.double()
    _close(_pointwise(x, w, bias, 1, sc, res), ref, 1e-5)
    _close(_pointwise(x, w, bias, 2), torch.sigmoid(x.double() @ w.t().double() + bias.double()), 1e-5)


def test_se_matches_torch():
    torch.manual_seed(3)
    B, H, W, Cc, Cs = 2, 13, 11, 96, 4
    x = torch.randn(B, H, W, Cc, device=DEV)
    w1, b1 = torch.randn(Cs, Cc, device=DEV) / 10, torch.randn(Cs, device=DEV)
    w2, b2 = torch.randn(Cc, Cs, device=DEV), torch.randn(Cc, device=DEV)
    part = torch.empty(capi.lib().stl_det_se_workspace(B) * Cc, device=DEV)
    sc = torch.empty(B, Cc, device=DEV)
    capi.call("stl_det_se", x.data_ptr(), B, H * W, Cc, Cs, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), part.data_ptr(),
              sc.data_ptr(), _st())
    m = x.mean((1, 2))
    ref = torch.sigmoid(F.silu(m @ w1.t() + b1) @ w2.t() + b2)
    _close(sc, ref, 1e-5)


def test_bifpn_node_and_zero_padded_pool():
    torch.manual_seed(5)
    B, Cc = 2, 16
    same = torch.randn(B, 8, 8, Cc, device=DEV)
    low = torch.randn(B, 4, 4, Cc, device=DEV)
    high = -torch.rand(B, 15, 15, Cc, device=DEV) - 0.1   # all negative: the zero padding decides every border maximum
    wparam = torch.tensor([0.7, -0.2, 1.3], device=DEV)
    f = capi.DetFuse()
    f.B, f.H, f.W, f.C, f.nterms = B, 8, 8, Cc, 3
    f.t[0] = capi.DetTerm(same.data_ptr(), 0, 8, 8, 0)
    f.t[1] = capi.DetTerm(low.data_ptr(), 1, 4, 4, 0)
    f.t[2] = capi.DetTerm(high.data_ptr(), 2, 15, 15, 0)
    f.wparam = wparam.data_ptr()
    out = torch.empty(B, 8, 8, Cc, device=DEV)
    f.out = out.data_ptr()
    capi.call("stl_det_fuse", C.byref(f), _st())
    nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
    w = F.relu(wparam)
    w = w / (w.sum() + 1e-4)
    pooled = R._pool(nchw(high))
    assert (pooled[..., -1, :] == 0).all() and (pooled[..., 0, :] == 0).all()   # border windows reach the zero padding
    ref = F.silu(w[0] * nchw(same) + w[1] * F.interpolate(nchw(low), scale_factor=2, mode="nearest") + w[2] * pooled)
    _close(nchw(out), ref, 1e-5)
    # even size: 1 pad after only
    g8 = torch.randn(B, 8, 8, Cc, device=DEV) - 3
    f2 = capi.DetFuse()
    f2.B, f2.H, f2.W, f2.C, f2.nterms = B, 4, 4, Cc, 1
    f2.t[0] = capi.DetTerm(g8.data_ptr(), 2, 8, 8, 0)
    o2 = torch.empty(B, 4, 4, Cc, device=DEV)
    f2.out = o2.data_ptr()
    capi.call("stl_det_fuse", C.byref(f2), _st())
    _close(nchw(o2), R._pool(nchw(g8)), 0)


def test_preprocess_matches_interpolate():
    m = E.setup_detector("efficientdet", "d0")
    ims = R.images()
    src = [torch.from_numpy(im).to(DEV) for im in ims]
    p, metas, _ = m._preprocess(src, 0, torch.device(DEV))
    for i, im in enumerate(ims):
        x = (torch.from_numpy(im).to(DEV).permute(2, 0, 1).float() / 255 - torch.tensor(E.MEAN, device=DEV)[:, None, None]) \
            / torch.tensor(E.STD, device=DEV)[:, None, None]
        nw, nh = metas[i][:2]
        ref = torch.zeros(3, 512, 512, device=DEV)
        ref[:, :nh, :nw] = F.interpolate(x[None], (nh, nw), mode="bilinear", align_corners=False)[0]
        _close(p.canvas[i].permute(2, 0, 1), ref, 1e-5)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def d0(g):
    m = E.setup_detector("efficientdet", "d0")
    m.load_state_dict(R.synth_state_dict(_layout(g, 0)), strict=True)
    return m.to(DEV)


def _chw():
    return [im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in R.images()]


def _ref_heads(g):
    reg = np.zeros((2, 49104, 4), np.float32)
    for i in range(2):
        reg[i, g[f"cand{i}_idx"]] = g[f"cand{i}_reg"]
    return reg, g["cls"]


def test_d0_against_reference(g, d0):
    feats, reg, cls, anc = d0(_chw(), postprocess=False)
    p = d0._plans[2]
    for i, t in enumerate(p.backbone):
        _close(t.permute(0, 3, 1, 2)[:, ::4, ::4, ::4], g[f"p{i + 3}_s"])
    for i, f in enumerate(feats):
        _close(f[:, ::4, ::4, ::4], g[f"f{i}_s"])
    _close(cls, g["cls"])
    for i in range(2):
        _close(reg[i, torch.from_numpy(g[f"cand{i}_idx"]).long().to(DEV)], g[f"cand{i}_reg"])
    np.testing.assert_allclose([reg.double().mean().item(), reg.double().std().item(), reg.double().abs().max().item()], g["reg_stats"],
                               rtol=1e-4, atol=1e-6)
    assert anc.shape == (1, 49104, 4)
    dets = d0(_chw())
    metas = [tuple(int(v) for v in m) for m in g["metas"]]
    # On the device's own head outputs the postprocess is exact (the device path against the restatement the reference is
    # pinned to).  Against the reference's detections: the reference's scores hold overlapping candidates whose scores differ
    # by less than 1e-5 (65 and 81 of 195 per image, detector_ref.near_ties); the network agrees to ~1e-6, so greedy NMS may
    # keep the other one of such a pair.  Every other detection must be the reference's, score within 1e-5, box within 1e-2 px.
    own = R.postprocess(E.anchors(0), reg.cpu().numpy(), cls.cpu().numpy(), 0.5, 0.5)
    rreg, rcls = _ref_heads(g)
    for i, d in enumerate(dets):
        assert d["boxes"].device.type == "cpu" and d["labels"].dtype == torch.int32 and d["boxes"].dtype == torch.float32
        ob, oc, os_ = own[i]
        np.testing.assert_array_equal(d["scores"].numpy(), os_)
        np.testing.assert_array_equal(d["labels"].numpy(), oc + 1)
        np.testing.assert_allclose(d["boxes"].numpy(), E.invert_affine(metas[i], ob), rtol=0, atol=1e-3)
        idx = np.nonzero(rcls[i].max(1) > 0.5)[0]
        cb, cs = R.decode(E.anchors(0), rreg[i])[idx], rcls[i][idx].max(1)
        tied = R.near_ties(cb, cs, np.zeros(len(idx), np.int64), 0.5)
        rb, rs = g[f"det{i}_boxes"], g[f"det{i}_scores"]
        gb, gs = d["boxes"].numpy(), d["scores"].numpy()
        for boxes_a, scores_a, boxes_b, scores_b in ((rb, rs, gb, gs), (gb, gs, rb, rs)):
            dist = np.abs(boxes_a[:, None, :] - boxes_b[None, :, :]).max(2)
            hit = dist.min(1) < 1e-2
            np.testing.assert_allclose(scores_b[dist.argmin(1)[hit]], scores_a[hit], rtol=0, atol=1e-5)
            for k in np.nonzero(~hit)[0]:   # an unmatched detection must be one of a near-tied pair of the reference's candidates
                j = np.argmin(np.abs(cs - scores_a[k]))
                assert abs(cs[j] - scores_a[k]) < 1e-5 and tied[j], (i, k, scores_a[k])


def test_detections_from_reference_heads_exact(g, d0):
    """decode + NMS on the device from the reference's own head outputs reproduce its detections exactly: the forward's dicts
    at threshold 0.5 (after invert_affine) and its postprocess at lo_thr, > 4096 candidates in image 0."""
    reg, cls = _ref_heads(g)
    an = torch.from_numpy(E.anchors(0)).to(DEV)
    r, c = torch.from_numpy(reg).to(DEV), torch.from_numpy(cls).to(DEV)
    metas = [tuple(int(v) for v in m) for m in g["metas"]]
    for i, (b, k, s) in enumerate(E.detect_from_heads(r, c, an, 0.5, 0.5)):
        np.testing.assert_array_equal(s, g[f"det{i}_scores"])
        np.testing.assert_array_equal(k.astype(np.int32) + 1, g[f"det{i}_labels"])
        np.testing.assert_allclose(E.invert_affine(metas[i], b), g[f"det{i}_boxes"], rtol=0, atol=1e-4)
    lo = float(g["lo_thr"])
    assert int((c[0].max(1)[0] > lo).sum()) > 4096
    for i, (b, k, s) in enumerate(E.detect_from_heads(r, c, an, lo, 0.5)):
        np.testing.assert_array_equal(s, g[f"lo{i}_scores"])
        np.testing.assert_array_equal(k, g[f"lo{i}_class_ids"])
        np.testing.assert_allclose(b, g[f"lo{i}_rois"], rtol=0, atol=1e-4)


def test_class_aware_nms_and_empty():
    torch.manual_seed(11)
    B, A, nc = 2, 49104, 3
    cls = torch.rand(B, A, nc, device=DEV) ** 4
    cls[1] = 0.01                                 # image 1: nothing passes
    reg = torch.randn(B, A, 4, device=DEV) * 0.2
    an = torch.from_numpy(E.anchors(0)).to(DEV)
    got = E.detect_from_heads(reg, cls, an, 0.6, 0.5)
    ref = R.postprocess(E.anchors(0), reg.cpu().numpy(), cls.cpu().numpy(), 0.6, 0.5)
    gb, gc, gs = got[0]
    rb, rc, rs = ref[0]
    assert len(np.unique(gc)) == 3
    np.testing.assert_array_equal(gc, rc)
    np.testing.assert_array_equal(gs, rs)
    np.testing.assert_allclose(gb, rb, rtol=0, atol=1e-4)
    assert got[1][0].shape == (0, 4)
    m = E.setup_detector("efficientdet", "d0").to(DEV)
    m.threshold = 1.01
    out = m(torch.rand(2, 3, 64, 80, device=DEV))
    for d in out:
        assert d["boxes"].shape == (0,) and d["labels"].shape == (0,) and d["scores"].shape == (0,)
        assert d["labels"].dtype == torch.int32


def test_bitwise_repeatable(d0):
    x = torch.from_numpy(np.stack(_chw()[:1])).to(DEV)
    a = [t.clone() for t in d0(x, postprocess=False)[1:3]]
    b = [t.clone() for t in d0(x, postprocess=False)[1:3]]
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_d3_stats(g):
    m = E.setup_detector("efficientdet", "d3")
    m.load_state_dict(R.synth_state_dict(_layout(g, 3)), strict=True)
    m = m.to(DEV)
    feats, reg, cls, _ = m(_chw()[:1], postprocess=False)
    for t, s in ((reg, g["d3_reg_stats"]), (cls, g["d3_cls_stats"])):
        st = np.array([t.double().mean().item(), t.double().std().item(), t.double().abs().max().item()])
        np.testing.assert_allclose(st, s, rtol=1e-3, atol=1e-4 * s[2])
    for f, s in zip(feats, g["d3_f_stats"]):
        st = np.array([f.double().mean().item(), f.double().std().item(), f.double().abs().max().item()])
        np.testing.assert_allclose(st, s, rtol=1e-3, atol=1e-4 * s[2])


def test_no_refold_without_change(d0):
    """Repeated calls reuse the packed weights and the plan, whichever way the device is named."""
    src = [torch.from_numpy(R.images()[0]).to(DEV)]
    p1, _ = d0.run_raw(src, 0, torch.device("cuda"))
    w1 = d0._wbuf
    p2, _ = d0.run_raw(src, 0, torch.device("cuda", torch.cuda.current_device()))
    assert p2 is p1 and d0._wbuf is w1


def test_refold_on_parameter_change(g):
    m = E.setup_detector("efficientdet", "d0")
    m.load_state_dict(R.synth_state_dict(_layout(g, 0)), strict=True)
    m = m.to(DEV)
    x = torch.from_numpy(np.stack(_chw()[:1])).to(DEV)
    c0 = m(x, postprocess=False)[2].clone()
    with torch.no_grad():
        m.classifier.header.pointwise_conv.conv.bias += 1.0
    c1 = m(x, postprocess=False)[2]
    assert (c1 > c0).all()


def test_detect_poses_equals_extractor(g, d0):
    from stlpose_amd import PoseHighResolutionNet
    from stlpose_amd.topdown import PoseExtractor, detect_poses
    from oracle import hrnet_ref
    ref = hrnet_ref.load_synth(hrnet_ref.RefPoseNet("tiny")).eval()
    net = PoseHighResolutionNet("tiny", "fp32")
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV).eval()
    ex = PoseExtractor(net, batch=8)
    ims = R.images()
    d0.threshold = 0.5
    got = detect_poses(d0, ex, ims, detector_thr=0.5)
    dets = d0([im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in ims])
    want = ex(ims, [d["boxes"] for d in dets], [d["scores"] for d in dets], [d["labels"].long() for d in dets], det_thr=0.5)
    for a, b in zip(got, want):
        assert len(a["boxes"]) > 0
        np.testing.assert_allclose(a["boxes"], b["boxes"], rtol=0, atol=1e-3)
        np.testing.assert_allclose(a["keypoints"], b["keypoints"], rtol=0, atol=1e-2 * max(1.0, np.abs(b["keypoints"]).max()))
