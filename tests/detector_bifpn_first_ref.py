"""The yardstick of the tests that train the FIRST BiFPN cell (``set_train_bifpn("all")``): cell 0 of
tests/detector_ref.eager_forward restated from the backbone's P3 / P4 / P5 (its helpers ``_conv``, ``_bn``, ``_same``, ``_sep``; the
pool, the upsampling and the fusion weights of tests/detector_bifpn_ref.py), evaluated in the dtype of what it is given and
differentiated by autograd; float64 is the yardstick, float32 the eager evaluation whose own error the bounds are scaled by.  The
cells behind it, the heads and the loss are those of tests/detector_bifpn_ref.py and tests/detector_train_ref.py.

Every pool takes its ROUTING from a given fp32 map -- the one the device stored -- for the reason stated in
tests/detector_bifpn_ref.py: the two unweighted pools (``t -> p6``, ``p6 -> p7``: border windows of a map with negative values are
won by the padding, exact ties among the 0 taps) and the four pooled node outputs.  With that no element is left out of any
comparison."""
from __future__ import annotations

import torch.nn.functional as F

from tests import detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR

CONVS = ("p5_to_p6", "p3_down_channel", "p4_down_channel", "p5_down_channel", "p4_down_channel_2", "p5_down_channel_2")
POOLED = ("t", "p6") + BR.POOLED   # the maps cell 0 pools: what its ``routes`` may hold


def cell0_forward(sd, p3, p4, p5, routes=None, pool=None):
    """Cell 0 from the NCHW backbone maps, detector_ref.eager_forward's lines for it -> {map name: map} with the five outputs under
    p3_out .. p7_out.  routes: {name in POOLED: the fp32 NCHW map whose winners route that map's pool} (absent: the map's own).
    pool: another pool(name, map) than the routed one (tools/detector_bifpn_bench.py times eager torch with detector_ref._pool)."""
    p, sw = "bifpn.0.", F.silu
    routes = routes or {}
    pool = pool or (lambda name, t: BR.routed_pool(t, routes.get(name)))
    layer = lambda key, x: R._bn(sd, p + key + ".1", R._conv(sd, p + key + ".0", x))  # noqa: E731
    up, o = BR.up, {}
    o["t"] = layer("p5_to_p6", p5)
    o["p6"] = pool("t", o["t"])
    o["p7"] = pool("p6", o["p6"])
    p3_in, p4_in, p5_in = layer("p3_down_channel", p3), layer("p4_down_channel", p4), layer("p5_down_channel", p5)
    w = BR.fusion_weights(sd[p + "p6_w1"])
    o["p6_up"] = R._sep(sd, p + "conv6_up", sw(w[0] * o["p6"] + w[1] * up(o["p7"])))
    w = BR.fusion_weights(sd[p + "p5_w1"])
    o["p5_up"] = R._sep(sd, p + "conv5_up", sw(w[0] * p5_in + w[1] * up(o["p6_up"])))
    w = BR.fusion_weights(sd[p + "p4_w1"])
    o["p4_up"] = R._sep(sd, p + "conv4_up", sw(w[0] * p4_in + w[1] * up(o["p5_up"])))
    w = BR.fusion_weights(sd[p + "p3_w1"])
    o["p3_out"] = R._sep(sd, p + "conv3_up", sw(w[0] * p3_in + w[1] * up(o["p4_up"])))
    p4_in, p5_in = layer("p4_down_channel_2", p4), layer("p5_down_channel_2", p5)
    w = BR.fusion_weights(sd[p + "p4_w2"])
    o["p4_out"] = R._sep(sd, p + "conv4_down", sw(w[0] * p4_in + w[1] * o["p4_up"] + w[2] * pool("p3_out", o["p3_out"])))
    w = BR.fusion_weights(sd[p + "p5_w2"])
    o["p5_out"] = R._sep(sd, p + "conv5_down", sw(w[0] * p5_in + w[1] * o["p5_up"] + w[2] * pool("p4_out", o["p4_out"])))
    w = BR.fusion_weights(sd[p + "p6_w2"])
    o["p6_out"] = R._sep(sd, p + "conv6_down", sw(w[0] * o["p6"] + w[1] * o["p6_up"] + w[2] * pool("p5_out", o["p5_out"])))
    w = BR.fusion_weights(sd[p + "p7_w2"])
    o["p7_out"] = R._sep(sd, p + "conv7_down", sw(w[0] * o["p7"] + w[1] * pool("p6_out", o["p6_out"])))
    return o


def method_yardstick(sd, cc, nc, ncells, p345, routes, anchors, gt, offsets, dtype, **kw):
    """detection_loss of the heads behind all `ncells` BiFPN cells run from the backbone's NCHW P3 / P4 / P5, in `dtype`; routes[j]:
    cell j's ``routes`` -> (classification, regression, {parameter: grad})."""
    st = BR.train_state(sd, range(ncells), dtype)
    p3, p4, p5 = (t.detach().cpu().to(dtype) for t in p345)
    levels = BR.levels_of(cell0_forward(st, p3, p4, p5, routes[0]))
    for j in range(1, ncells):
        levels = BR.levels_of(BR.cell_forward(st, j, levels, routes[j]))
    reg, cls = TR.heads_forward(st, cc, nc, levels)
    c, r, _, _ = TR.detection_loss(reg, cls, anchors, gt, offsets, **kw)
    (c + r).backward()
    return c.detach(), r.detach(), {k: v.grad for k, v in st.items() if v.requires_grad}


def tensor_class(name: str) -> str:
    """The class of a cell-0 parameter in the measured-ratio table: the four of detector_bifpn_ref.tensor_class for the eight
    nodes, first_conv / first_bn for the six 1x1 layers on the backbone maps."""
    key = name.split(".")[2]
    if key in CONVS:
        return "first_conv" if ".0.conv." in name else "first_bn"
    return BR.tensor_class(name)
