"""Restatements for the EfficientDet detector tests: the seeded synthetic weights, cv2.resize(INTER_LINEAR) on float32, the
postprocess with torchvision 0.4's batched_nms / nms (numpy, float32), and an eager torch forward of the network (F.conv2d on
the reference's state_dict, NCHW) -- what the GPU results, the fixture generator and tools/detector_bench.py hold to."""
from __future__ import annotations

import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.topdown_ref import nms  # noqa: F401  (torchvision.ops.nms restatement)

# classifier header: weights scaled by CLS_GAIN and bias CLS_BIAS, so that a few hundred anchors per image score above 0.5 and
# thousands above 0.2 with the synthetic weights
CLS_GAIN, CLS_BIAS = 30.0, -3.95


def _rng(key: str, seed: int) -> np.random.Generator:
    h = int.from_bytes(hashlib.sha256(f"{seed}:{key}".encode()).digest()[:8], "little")
    return np.random.Generator(np.random.PCG64(h))


def synth_state_dict(shapes, seed: int = 15) -> dict:
    """{key: tensor} for {key: shape}: convs ~ N(0, 1 / fan_in), biases N(0, 0.05), BN weight U(0.7, 1.3), bias N(0, 0.1), running
    mean N(0, 0.1), running var U(0.6, 1.4), BiFPN weights U(0.3, 1.7), the classifier header as CLS_GAIN / CLS_BIAS say."""
    sd = {}
    bns = {k[:-len(".running_mean")] for k in shapes if k.endswith(".running_mean")}
    for k, shp in shapes.items():
        r = _rng(k, seed)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.int64)
            continue
        if len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            v = r.normal(0, 1.0 / math.sqrt(fan_in), shp)
        elif "_w1" in k or "_w2" in k:
            v = r.uniform(0.3, 1.7, shp)
        elif k.endswith("running_mean"):
            v = r.normal(0, 0.1, shp)
        elif k.endswith("running_var"):
            v = r.uniform(0.6, 1.4, shp)
        elif k.rsplit(".", 1)[0] in bns:
            v = r.uniform(0.7, 1.3, shp) if k.endswith("weight") else r.normal(0, 0.1, shp)
        else:
            v = r.normal(0, 0.05, shp)
        if k == "classifier.header.pointwise_conv.conv.bias":
            v = np.full(shp, CLS_BIAS)
        if k == "classifier.header.pointwise_conv.conv.weight":
            v = v * CLS_GAIN
        sd[k] = torch.from_numpy(np.asarray(v, np.float32))
    return sd


SIZES = ((300, 400), (480, 360))


def images():
    """The fixture's two uint8 HWC RGB test images (300 x 400 and 480 x 360), from a seed."""
    rng = np.random.default_rng(1501)
    out = []
    for h, w in SIZES:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        base = 127 + 60 * np.sin(xx / 23.0)[..., None] * np.cos(yy / 31.0)[..., None] * np.array([1.0, 0.6, -0.8])
        img = base + rng.normal(0, 25, (h, w, 3))
        for _ in range(6):   # a few bright blocks: structure for the detector to respond to
            y0, x0 = rng.integers(0, h - 60), rng.integers(0, w - 40)
            img[y0:y0 + rng.integers(30, 60), x0:x0 + rng.integers(20, 40)] = rng.uniform(0, 255, 3)
        out.append(np.clip(np.round(img), 0, 255).astype(np.uint8))
    return out


# ------------------------------------------------------------------------------------------------ preprocess
def resize_linear(img_hwc: np.ndarray, new_w: int, new_h: int) -> np.ndarray:
    """cv2.resize(img, (new_w, new_h)) INTER_LINEAR on float32 HWC: src = (dst + 0.5) * (old / new) - 0.5 in double, rounded to
    float, floored; out-of-range taps clamp to the edge pixel with weight 1; x first within a row, then the rows."""
    h, w = img_hwc.shape[:2]

    def taps(n_out, n_in):
        scale = 1.0 / (n_out / n_in)
        f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        a = (f - i.astype(np.float32)).astype(np.float32)
        lo = i < 0
        i[lo], a[lo] = 0, 0
        hi = i >= n_in - 1
        i[hi], a[hi] = n_in - 1, 0
        return i, np.minimum(i + 1, n_in - 1), (np.float32(1) - a).astype(np.float32), a
    y0, y1, wy0, wy1 = taps(new_h, h)
    x0, x1, wx0, wx1 = taps(new_w, w)
    x = img_hwc.astype(np.float32)
    top = x[y0][:, x0] * wx0[None, :, None] + x[y0][:, x1] * wx1[None, :, None]
    bot = x[y1][:, x0] * wx0[None, :, None] + x[y1][:, x1] * wx1[None, :, None]
    return (top * wy0[:, None, None] + bot * wy1[:, None, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ postprocess
def batched_nms(boxes, scores, idxs, iou_thr):
    """torchvision 0.4 batched_nms: boxes + idxs * (boxes.max() + 1), then nms."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    if len(b) == 0:
        return np.zeros(0, np.int64)
    off = np.asarray(idxs, np.float32) * (b.max() + np.float32(1))
    return nms(b + off[:, None], scores, iou_thr)


def decode(anchors, reg, size=512):
    """BBoxTransform + ClipBoxes (efficientdet_utils/utils.py:14-56) in numpy float32: anchors [A, 4] (y1, x1, y2, x2), reg
    [A, 4] (dy, dx, dh, dw) -> boxes [A, 4] (x1, y1, x2, y2) clipped to the size x size canvas."""
    a = np.asarray(anchors, np.float32).reshape(-1, 4)
    reg = np.asarray(reg, np.float32)
    yca, xca = (a[:, 0] + a[:, 2]) / np.float32(2), (a[:, 1] + a[:, 3]) / np.float32(2)
    ha, wa = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    w, h = np.exp(reg[:, 3]) * wa, np.exp(reg[:, 2]) * ha
    yc, xc = reg[:, 0] * ha + yca, reg[:, 1] * wa + xca
    bx = np.stack([xc - w / np.float32(2), yc - h / np.float32(2), xc + w / np.float32(2), yc + h / np.float32(2)], 1)
    bx[:, 0] = np.maximum(bx[:, 0], 0)
    bx[:, 1] = np.maximum(bx[:, 1], 0)
    bx[:, 2] = np.minimum(bx[:, 2], np.float32(size - 1))
    bx[:, 3] = np.minimum(bx[:, 3], np.float32(size - 1))
    return bx


def near_ties(boxes, scores, classes, iou_thr, eps=1e-5):
    """[n] bool: candidates with an overlapping (IoU > iou_thr - 1e-4) candidate of their class whose score differs by less than
    eps -- the ones whose fate greedy NMS decides by rounding when two implementations agree only to ~1e-6."""
    b = np.asarray(boxes, np.float32)
    n = len(b)
    x1 = np.maximum(b[:, None, 0], b[None, :, 0])
    y1 = np.maximum(b[:, None, 1], b[None, :, 1])
    x2 = np.minimum(b[:, None, 2], b[None, :, 2])
    y2 = np.minimum(b[:, None, 3], b[None, :, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iou = inter / (area[:, None] + area[None, :] - inter)
    s = np.asarray(scores, np.float32)
    c = np.asarray(classes)
    pair = (c[:, None] == c[None, :]) & ~np.eye(n, dtype=bool) & (iou > iou_thr - 1e-4) & (np.abs(s[:, None] - s[None, :]) < eps)
    return pair.any(1)


def postprocess(anchors, regression, classification, threshold, iou_thr, size=512):
    """efficientdet_utils/utils.py:14-56, 150-187 in numpy float32: per image (rois [k, 4], class_ids [k], scores [k])."""
    out = []
    for reg, cls in zip(np.asarray(regression, np.float32), np.asarray(classification, np.float32)):
        bx = decode(anchors, reg, size)
        sc = cls.max(1)
        m = sc > np.float32(threshold)
        if not m.any():
            out.append((np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float32)))
            continue
        cl = cls[m].argmax(1)
        keep = batched_nms(bx[m], sc[m], cl, iou_thr)
        out.append((bx[m][keep], cl[keep].astype(np.int64), sc[m][keep]))
    return out


# ------------------------------------------------------------------------------------------------ eager forward (NCHW)
def _same(x, k, s):
    h, w = x.shape[-2:]
    ev = (math.ceil(h / s) - 1) * s - h + k
    eh = (math.ceil(w / s) - 1) * s - w + k
    return F.pad(x, [eh // 2, eh - eh // 2, ev // 2, ev - ev // 2])


def _conv(sd, p, x, k=1, s=1, groups=1):
    return F.conv2d(_same(x, k, s), sd[p + ".conv.weight"], sd.get(p + ".conv.bias"), s, 0, 1, groups)


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-3)


def _pool(x):
    return F.max_pool2d(_same(x, 3, 2), 3, 2)


def _sep(sd, p, x, norm=True):
    c = x.shape[1]
    x = _conv(sd, p + ".pointwise_conv", _conv(sd, p + ".depthwise_conv", x, 3, 1, c))
    return _bn(sd, p + ".bn", x) if norm else x


def eager_forward(sd, cc: int, nc: int, x: torch.Tensor):
    """The network on the NCHW canvas x with the reference's state_dict sd -> (five NCHW features, regression, classification)."""
    from stlpose_amd.efficientdet import FPN_REPEATS, HEAD_REPEATS, block_specs
    sw = F.silu
    pre = "backbone_net.model."
    x = sw(_bn(sd, pre + "_bn0", _conv(sd, pre + "_conv_stem", x, 3, 2)))
    feats = []
    specs = block_specs(cc)
    for i, b in enumerate(specs):
        if b["s"] == 2:
            feats.append(x)
        p = pre + f"_blocks.{i}."
        inp = x
        if b["e"] != 1:
            x = sw(_bn(sd, p + "_bn0", _conv(sd, p + "_expand_conv", x)))
        x = sw(_bn(sd, p + "_bn1", _conv(sd, p + "_depthwise_conv", x, b["k"], b["s"], x.shape[1])))
        q = F.adaptive_avg_pool2d(x, 1)
        q = _conv(sd, p + "_se_expand", sw(_conv(sd, p + "_se_reduce", q)))
        x = torch.sigmoid(q) * x
        x = _bn(sd, p + "_bn2", _conv(sd, p + "_project_conv", x))
        if b["skip"]:
            x = x + inp
    feats.append(x)
    p3, p4, p5 = feats[-3:]
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
    levels = None
    for j in range(FPN_REPEATS[cc]):
        p = f"bifpn.{j}."

        def wt(n):
            w = F.relu(sd[p + n])
            return w / (torch.sum(w, dim=0) + 1e-4)
        if j == 0:
            p6_in = _pool(_bn(sd, p + "p5_to_p6.1", _conv(sd, p + "p5_to_p6.0", p5)))
            p7_in = _pool(p6_in)
            p3_in = _bn(sd, p + "p3_down_channel.1", _conv(sd, p + "p3_down_channel.0", p3))
            p4_in = _bn(sd, p + "p4_down_channel.1", _conv(sd, p + "p4_down_channel.0", p4))
            p5_in = _bn(sd, p + "p5_down_channel.1", _conv(sd, p + "p5_down_channel.0", p5))
        else:
            p3_in, p4_in, p5_in, p6_in, p7_in = levels
        w = wt("p6_w1")
        p6_up = _sep(sd, p + "conv6_up", sw(w[0] * p6_in + w[1] * up(p7_in)))
        w = wt("p5_w1")
        p5_up = _sep(sd, p + "conv5_up", sw(w[0] * p5_in + w[1] * up(p6_up)))
        w = wt("p4_w1")
        p4_up = _sep(sd, p + "conv4_up", sw(w[0] * p4_in + w[1] * up(p5_up)))
        w = wt("p3_w1")
        p3_out = _sep(sd, p + "conv3_up", sw(w[0] * p3_in + w[1] * up(p4_up)))
        if j == 0:
            p4_in = _bn(sd, p + "p4_down_channel_2.1", _conv(sd, p + "p4_down_channel_2.0", p4))
            p5_in = _bn(sd, p + "p5_down_channel_2.1", _conv(sd, p + "p5_down_channel_2.0", p5))
        w = wt("p4_w2")
        p4_out = _sep(sd, p + "conv4_down", sw(w[0] * p4_in + w[1] * p4_up + w[2] * _pool(p3_out)))
        w = wt("p5_w2")
        p5_out = _sep(sd, p + "conv5_down", sw(w[0] * p5_in + w[1] * p5_up + w[2] * _pool(p4_out)))
        w = wt("p6_w2")
        p6_out = _sep(sd, p + "conv6_down", sw(w[0] * p6_in + w[1] * p6_up + w[2] * _pool(p5_out)))
        w = wt("p7_w2")
        p7_out = _sep(sd, p + "conv7_down", sw(w[0] * p7_in + w[1] * _pool(p6_out)))
        levels = (p3_out, p4_out, p5_out, p6_out, p7_out)
    outs = []
    for head, k in (("regressor", 4), ("classifier", nc)):
        fs = []
        for lv, f in enumerate(levels):
            for i in range(HEAD_REPEATS[cc]):
                f = sw(_bn(sd, f"{head}.bn_list.{lv}.{i}", _sep(sd, f"{head}.conv_list.{i}", f, norm=False)))
            f = _sep(sd, f"{head}.header", f, norm=False)
            fs.append(f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, k))
        outs.append(torch.cat(fs, 1))
    return levels, outs[0], torch.sigmoid(outs[1])
