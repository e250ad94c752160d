"""The yardstick of the BiFPN fine-tuning tests: one non-first BiFPN cell of tests/detector_ref.eager_forward restated from its five
inputs (its helpers ``_sep``, ``_same``, ``_bn``), evaluated in the dtype of what it is given and differentiated by autograd;
float64 is the yardstick, float32 the eager evaluation whose own error the bounds are scaled by.

The pooled terms have near-ties, and an independent fp64 forward picks other winners than the fp32 one (for D0 with the synthetic
weights at batch 2 the two evaluations of eager_forward disagree on 51 pool winners, and thousands of windows have exactly equal
top values, e.g. border windows won by the padding).  A flipped winner moves a gradient to a neighbouring pixel, far outside any
fp32 error bar.  So the pool here takes its ROUTING from a given fp32 map -- the one the device stored -- and applies it to its own
values (``routed_pool``): torch's CPU max_pool2d takes the first maximum in scan order too, with the explicit zero padding in
place.  With that no element is left out of any comparison."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import detector_ref as R, detector_train_ref as TR

POOLED = ("p3_out", "p4_out", "p5_out", "p6_out")   # the maps a cell pools: what ``routes`` may hold


def routed_pool(x, route32=None):
    """MaxPool2dStaticSamePadding(3, 2) of the NCHW map x whose winners are those of the fp32 map route32 (None: x's own): the
    zero-padded map, max_pool2d's indices of the padded route, x's padded values gathered at them."""
    route = x.detach() if route32 is None else route32.to(torch.float32)
    _, idx = F.max_pool2d(R._same(route, 3, 2), 3, 2, return_indices=True)
    return R._same(x, 3, 2).flatten(2).gather(2, idx.flatten(2)).view(idx.shape)


def up(t, h=None, w=None):
    """nearest x2, cut to h x w (an odd output)"""
    t = F.interpolate(t, scale_factor=2, mode="nearest")
    return t if h is None else t[..., :h, :w]


def fusion_weights(p):
    w = F.relu(p)
    return w / (torch.sum(w, dim=0) + 1e-4)


def cell_forward(sd, j: int, ins, routes=None, pool=None):
    """Cell j > 0 from its five NCHW inputs (p3 .. p7), detector_ref.eager_forward's lines for it -> {map name: map} with the five
    outputs under p3_out .. p7_out.  routes: {name in POOLED: the fp32 NCHW map whose winners route that map's pool}.  pool: another
    pool(name, map) than the routed one (tools/detector_bifpn_bench.py times eager torch with detector_ref._pool)."""
    p, sw = f"bifpn.{j}.", F.silu
    routes = routes or {}
    pool = pool or (lambda name, t: routed_pool(t, routes.get(name)))
    p3_in, p4_in, p5_in, p6_in, p7_in = ins
    o = {}
    w = fusion_weights(sd[p + "p6_w1"])
    o["p6_up"] = R._sep(sd, p + "conv6_up", sw(w[0] * p6_in + w[1] * up(p7_in)))
    w = fusion_weights(sd[p + "p5_w1"])
    o["p5_up"] = R._sep(sd, p + "conv5_up", sw(w[0] * p5_in + w[1] * up(o["p6_up"])))
    w = fusion_weights(sd[p + "p4_w1"])
    o["p4_up"] = R._sep(sd, p + "conv4_up", sw(w[0] * p4_in + w[1] * up(o["p5_up"])))
    w = fusion_weights(sd[p + "p3_w1"])
    o["p3_out"] = R._sep(sd, p + "conv3_up", sw(w[0] * p3_in + w[1] * up(o["p4_up"])))
    w = fusion_weights(sd[p + "p4_w2"])
    o["p4_out"] = R._sep(sd, p + "conv4_down", sw(w[0] * p4_in + w[1] * o["p4_up"] + w[2] * pool("p3_out", o["p3_out"])))
    w = fusion_weights(sd[p + "p5_w2"])
    o["p5_out"] = R._sep(sd, p + "conv5_down", sw(w[0] * p5_in + w[1] * o["p5_up"] + w[2] * pool("p4_out", o["p4_out"])))
    w = fusion_weights(sd[p + "p6_w2"])
    o["p6_out"] = R._sep(sd, p + "conv6_down", sw(w[0] * p6_in + w[1] * o["p6_up"] + w[2] * pool("p5_out", o["p5_out"])))
    w = fusion_weights(sd[p + "p7_w2"])
    o["p7_out"] = R._sep(sd, p + "conv7_down", sw(w[0] * p7_in + w[1] * pool("p6_out", o["p6_out"])))
    return o


def levels_of(o):
    return [o[k] for k in ("p3_out", "p4_out", "p5_out", "p6_out", "p7_out")]


def train_state(sd, cells, dtype):
    """The entries of the given BiFPN cells and of regressor.* / classifier.* in `dtype`; the parameters require grad."""
    pre = tuple(f"bifpn.{j}." for j in cells) + ("regressor.", "classifier.")
    out = {}
    for k, v in sd.items():
        if k.startswith(pre) and not k.endswith("num_batches_tracked"):
            t = v.detach().cpu().to(dtype).clone()
            out[k] = t if k.endswith(("running_mean", "running_var")) else t.requires_grad_(True)
    return out


def method_yardstick(sd, cc, nc, cells, ins, routes, anchors, gt, offsets, dtype, **kw):
    """detection_loss of the heads behind the BiFPN cells `cells` (consecutive, ending with the last) run from the first one's five
    NCHW inputs, in `dtype`; routes[j]: cell j's ``routes`` -> (classification, regression, {parameter: grad})."""
    st = train_state(sd, cells, dtype)
    levels = [t.detach().cpu().to(dtype) for t in ins]
    for j in cells:
        levels = levels_of(cell_forward(st, j, levels, routes[j]))
    reg, cls = TR.heads_forward(st, cc, nc, levels)
    c, r, _, _ = TR.detection_loss(reg, cls, anchors, gt, offsets, **kw)
    (c + r).backward()
    return c.detach(), r.detach(), {k: v.grad for k, v in st.items() if v.requires_grad}


def tensor_class(name: str) -> str:
    """The class of a trainable-cell parameter in the measured-ratio table: depthwise, pointwise, bn or fusion."""
    if "depthwise_conv" in name:
        return "depthwise"
    if "pointwise_conv" in name:
        return "pointwise"
    return "bn" if ".bn." in name else "fusion"
