"""The detector's 16-bit compute modes restated on top of tests/detector_ref.py: ``forward16`` is ``detector_ref.eager_forward``
with a ``store(t)`` hook at every point where the device plan (stlpose_amd.efficientdet._Plan) writes a 16-bit tensor, and, with a
``dtype``, the BN-folded pointwise weights rounded once to that type as the packer does.

  store = identity, dtype = None          -> detector_ref.eager_forward, bit for bit (the same calls in the same order)
  store = lambda t: t.to(dtype).float()   -> the storage-rounding emulation: what 16-bit storage costs the reference's own arithmetic

All arithmetic between two stores is fp32 (torch's convs) or fp64 (the BN fold).  Where the device keeps fp32 it stays fp32 here:
the canvas, depthwise weights, every bias, the squeeze-excitation branch (pooled from the depthwise output before it is rounded,
as the depthwise kernel does), the attention weights and the head outputs."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import detector_ref as R


def identity(t):
    return t


def rounder(dtype):
    return lambda t: t.to(dtype).float()


def _pw(sd, conv, bn, x, dtype):
    """1x1 conv ``conv`` (+ BN ``bn`` or None) on x.  dtype None: the reference's conv then BN.  Otherwise BN folded into the
    weights in fp64 (efficientdet._Packer.pw), the weights rounded to dtype, the bias fp32."""
    if dtype is None:
        y = R._conv(sd, conv, x)
        return y if bn is None else R._bn(sd, bn, y)
    w = sd[conv + ".conv.weight"].double()
    b = sd[conv + ".conv.bias"].double() if conv + ".conv.bias" in sd else None
    if bn is not None:
        s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-3)
        t = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s
        w = w * s[:, None, None, None]
        b = t if b is None else b * s + t
    return F.conv2d(x, w.to(dtype).float(), None if b is None else b.float())


def _sep(sd, p, x, store, dtype, bn="own"):
    """SeparableConvBlock: depthwise (stored), pointwise with its own BN, another BN (the heads' bn_list) or none."""
    c = x.shape[1]
    d = store(R._conv(sd, p + ".depthwise_conv", x, 3, 1, c))
    return _pw(sd, p + ".pointwise_conv", p + ".bn" if bn == "own" else bn, d, dtype)


def forward16(sd, cc: int, nc: int, x: torch.Tensor, store=identity, dtype=None):
    """(five NCHW features, regression, classification) as detector_ref.eager_forward returns them."""
    from stlpose_amd.efficientdet import FPN_REPEATS, HEAD_REPEATS, block_specs
    sw = F.silu
    pre = "backbone_net.model."
    x = store(sw(R._bn(sd, pre + "_bn0", R._conv(sd, pre + "_conv_stem", x, 3, 2))))
    feats = []
    specs = block_specs(cc)
    for i, b in enumerate(specs):
        if b["s"] == 2:
            feats.append(x)
        p = pre + f"_blocks.{i}."
        inp = x
        if b["e"] != 1:
            x = store(sw(_pw(sd, p + "_expand_conv", p + "_bn0", x, dtype)))
        x = sw(R._bn(sd, p + "_bn1", R._conv(sd, p + "_depthwise_conv", x, b["k"], b["s"], x.shape[1])))
        q = F.adaptive_avg_pool2d(x, 1)   # from the values before rounding
        x = store(x)
        q = R._conv(sd, p + "_se_expand", sw(R._conv(sd, p + "_se_reduce", q)))
        x = store(torch.sigmoid(q) * x)   # the pointwise kernel's operand: scaled in fp32, rounded once
        x = _pw(sd, p + "_project_conv", p + "_bn2", x, dtype)
        if b["skip"]:
            x = x + inp
        x = store(x)
    feats.append(x)
    p3, p4, p5 = feats[-3:]
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
    pool = R._pool   # a maximum of stored values (or the padding's 0) is a stored value: nothing to round
    levels = None
    for j in range(FPN_REPEATS[cc]):
        p = f"bifpn.{j}."

        def wt(n):
            w = F.relu(sd[p + n])
            return w / (torch.sum(w, dim=0) + 1e-4)

        def node(name, t):
            return store(_sep(sd, p + name, store(sw(t)), store, dtype))
        if j == 0:
            p6_in = pool(store(_pw(sd, p + "p5_to_p6.0", p + "p5_to_p6.1", p5, dtype)))
            p7_in = pool(p6_in)
            p3_in = store(_pw(sd, p + "p3_down_channel.0", p + "p3_down_channel.1", p3, dtype))
            p4_in = store(_pw(sd, p + "p4_down_channel.0", p + "p4_down_channel.1", p4, dtype))
            p5_in = store(_pw(sd, p + "p5_down_channel.0", p + "p5_down_channel.1", p5, dtype))
        else:
            p3_in, p4_in, p5_in, p6_in, p7_in = levels
        w = wt("p6_w1")
        p6_up = node("conv6_up", w[0] * p6_in + w[1] * up(p7_in))
        w = wt("p5_w1")
        p5_up = node("conv5_up", w[0] * p5_in + w[1] * up(p6_up))
        w = wt("p4_w1")
        p4_up = node("conv4_up", w[0] * p4_in + w[1] * up(p5_up))
        w = wt("p3_w1")
        p3_out = node("conv3_up", w[0] * p3_in + w[1] * up(p4_up))
        if j == 0:
            p4_in = store(_pw(sd, p + "p4_down_channel_2.0", p + "p4_down_channel_2.1", p4, dtype))
            p5_in = store(_pw(sd, p + "p5_down_channel_2.0", p + "p5_down_channel_2.1", p5, dtype))
        w = wt("p4_w2")
        p4_out = node("conv4_down", w[0] * p4_in + w[1] * p4_up + w[2] * pool(p3_out))
        w = wt("p5_w2")
        p5_out = node("conv5_down", w[0] * p5_in + w[1] * p5_up + w[2] * pool(p4_out))
        w = wt("p6_w2")
        p6_out = node("conv6_down", w[0] * p6_in + w[1] * p6_up + w[2] * pool(p5_out))
        w = wt("p7_w2")
        p7_out = node("conv7_down", w[0] * p7_in + w[1] * pool(p6_out))
        levels = (p3_out, p4_out, p5_out, p6_out, p7_out)
    outs = []
    for head, k in (("regressor", 4), ("classifier", nc)):
        fs = []
        for lv, f in enumerate(levels):
            for i in range(HEAD_REPEATS[cc]):
                f = store(sw(_sep(sd, f"{head}.conv_list.{i}", f, store, dtype, bn=f"{head}.bn_list.{lv}.{i}")))
            f = _sep(sd, f"{head}.header", f, store, dtype, bn=None)   # the header writes fp32
            fs.append(f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, k))
        outs.append(torch.cat(fs, 1))
    return levels, outs[0], torch.sigmoid(outs[1])


def rel_err(a, y) -> float:
    """max|a - y| / max|y|, in fp64."""
    a, y = torch.as_tensor(a).double().cpu(), torch.as_tensor(y).double().cpu()
    return ((a - y).abs().max() / y.abs().max()).item()


def canvas() -> torch.Tensor:
    """detector_ref.images() preprocessed on the host: the normalised, resized 512 x 512 canvases, NCHW float32."""
    import numpy as np

    from stlpose_amd import efficientdet as E
    out = []
    for im in R.images():
        x = (im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - np.array(E.MEAN, np.float32)[:, None, None]) \
            / np.array(E.STD, np.float32)[:, None, None]
        nw, nh = E.resize_meta(*im.shape[:2])[:2]
        c = np.zeros((E.MAX_SIZE, E.MAX_SIZE, 3), np.float32)
        c[:nh, :nw] = R.resize_linear(x.transpose(1, 2, 0), nw, nh)
        out.append(c.transpose(2, 0, 1))
    return torch.from_numpy(np.stack(out))
