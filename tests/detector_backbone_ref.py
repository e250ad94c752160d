"""The yardstick of the tests that train the backbone's LAST STAGE (``set_train_backbone(k)``): the trainable MBConv blocks of
tests/detector_ref.eager_forward restated from the first one's input (its helpers ``_conv``, ``_bn``), evaluated in the dtype of what
it is given and differentiated by autograd; float64 is the yardstick, float32 the eager evaluation whose own error the bounds are
scaled by.  BN runs on its running statistics and there is no drop-connect.  Behind the blocks: the first BiFPN cell of
tests/detector_bifpn_first_ref.py from the stored P3 and P4 and the blocks' own P5, the other cells, the heads and the loss of
tests/detector_bifpn_ref.py and tests/detector_train_ref.py, every pool routed by the device's stored map (the reason is stated in
tests/detector_bifpn_ref.py).

``detach_gate``: the same graph with the squeeze-excitation gate held constant -- what a backward without the gate path computes.  The
tests assert that the device differs from it by more than its bound, so they can see a missing gate path."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import detector_bifpn_first_ref as FR, detector_bifpn_ref as BR, detector_ref as R, detector_train_ref as TR

PRE = "backbone_net.model._blocks."


def block_forward(sd, i: int, spec: dict, x, detach_gate: bool = False):
    """MBConv block i (an expanding one) on the NCHW map x: detector_ref.eager_forward's lines for it."""
    p, sw = f"{PRE}{i}.", F.silu
    inp = x
    x = sw(R._bn(sd, p + "_bn0", R._conv(sd, p + "_expand_conv", x)))
    x = sw(R._bn(sd, p + "_bn1", R._conv(sd, p + "_depthwise_conv", x, spec["k"], spec["s"], x.shape[1])))
    q = F.adaptive_avg_pool2d(x, 1)
    q = R._conv(sd, p + "_se_expand", sw(R._conv(sd, p + "_se_reduce", q)))
    g = torch.sigmoid(q)
    x = (g.detach() if detach_gate else g) * x
    x = R._bn(sd, p + "_bn2", R._conv(sd, p + "_project_conv", x))
    return x + inp if spec["skip"] else x


def train_state(sd, blocks, ncells, dtype):
    """The entries of the given blocks, of every BiFPN cell and of the heads in `dtype`; the parameters require grad."""
    out = BR.train_state(sd, range(ncells), dtype)
    pre = tuple(f"{PRE}{i}." for i in blocks)
    for k, v in sd.items():
        if k.startswith(pre) and not k.endswith("num_batches_tracked"):
            t = v.detach().cpu().to(dtype).clone()
            out[k] = t if k.endswith(("running_mean", "running_var")) else t.requires_grad_(True)
    return out


def method_yardstick(sd, cc, nc, ncells, blocks, x_in, p34, routes, anchors, gt, offsets, dtype, detach_gate=False, **kw):
    """detection_loss of the heads behind all `ncells` BiFPN cells behind the MBConv blocks `blocks` (consecutive indices ending with
    the last block), run from the first of these blocks' NCHW input x_in and the stored NCHW P3 / P4 (p34), in `dtype`; routes[j]: cell
    j's ``routes`` -> (classification, regression, {parameter: grad}); a parameter the loss does not reach has a zero gradient."""
    from stlpose_amd.efficientdet import block_specs
    specs = block_specs(cc)
    st = train_state(sd, blocks, ncells, dtype)
    x = x_in.detach().cpu().to(dtype)
    for i in blocks:
        x = block_forward(st, i, specs[i], x, detach_gate)
    p3, p4 = (t.detach().cpu().to(dtype) for t in p34)
    levels = BR.levels_of(FR.cell0_forward(st, p3, p4, x, routes[0]))
    for j in range(1, ncells):
        levels = BR.levels_of(BR.cell_forward(st, j, levels, routes[j]))
    reg, cls = TR.heads_forward(st, cc, nc, levels)
    c, r, _, _ = TR.detection_loss(reg, cls, anchors, gt, offsets, **kw)
    (c + r).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in st.items() if v.requires_grad}
    return c.detach(), r.detach(), grads


CLASSES = ("expand", "expand_bn", "depthwise", "depthwise_bn", "se", "project", "project_bn")


def tensor_class(name: str) -> str:
    """The class of a trainable-block parameter in the measured-ratio table (CLASSES)."""
    key = name[len(PRE):].split(".")[1]
    return {"_expand_conv": "expand", "_bn0": "expand_bn", "_depthwise_conv": "depthwise", "_bn1": "depthwise_bn", "_se_reduce": "se",
            "_se_expand": "se", "_project_conv": "project", "_bn2": "project_bn"}[key]
