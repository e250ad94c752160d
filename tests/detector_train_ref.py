"""The yardstick of the detector fine-tuning tests: the RetinaNet / EfficientDet detection loss (focal classification + smooth-L1
box regression over IoU-assigned anchors, as include/stlpose_hip.h states it at stl_det_loss) and the heads of
tests/detector_ref.eager_forward run from given features, in plain torch, differentiated by autograd.  Every function works in
the dtype of what it is given: float64 is the yardstick, float32 the eager evaluation whose own error the bounds are scaled by."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import detector_ref as R


def iou_matrix(anchors, gt):
    """anchors [A, 4] (y1, x1, y2, x2), gt [G, >= 4] (x1, y1, x2, y2) -> [A, G]"""
    ay1, ax1, ay2, ax2 = (anchors[:, i, None] for i in range(4))
    gx1, gy1, gx2, gy2 = (gt[None, :, i] for i in range(4))
    iw = (torch.minimum(ax2, gx2) - torch.maximum(ax1, gx1)).clamp(min=0)
    ih = (torch.minimum(ay2, gy2) - torch.maximum(ay1, gy1)).clamp(min=0)
    inter = iw * ih
    return inter / ((ax2 - ax1) * (ay2 - ay1) + (gx2 - gx1) * (gy2 - gy1) - inter).clamp(min=1e-8)


def assign(anchors, gt):
    """-> (state [A]: 1 positive, 0 negative, -1 ignored; g* [A]: the first argmax; m [A]: the max IoU)"""
    A = anchors.shape[0]
    if gt.shape[0] == 0:
        z = torch.zeros(A, dtype=torch.long)
        return z, z, torch.zeros(A, dtype=anchors.dtype)
    iou = iou_matrix(anchors, gt)
    m, g = iou.max(1)
    g = (iou == m[:, None]).long().argmax(1)   # the first maximum
    state = torch.where(m >= 0.5, 1, torch.where(m < 0.4, 0, -1))
    return state, g, m


def detection_loss(reg, cls, anchors, gt, offsets, alpha=0.25, gamma=2.0, box_weight=50.0):
    """reg [B, A, 4], cls [B, A, nc] (after the sigmoid), anchors [A, 4], gt [sum G, 5], offsets [B + 1] ->
    (classification, regression, N_pos per image, state [B, A])."""
    B, A, nc = cls.shape
    dt = reg.dtype
    anchors, gt = anchors.to(dt), gt.to(dt)
    wa, ha = anchors[:, 3] - anchors[:, 1], anchors[:, 2] - anchors[:, 0]
    cxa, cya = anchors[:, 1] + 0.5 * wa, anchors[:, 0] + 0.5 * ha
    lc, lr, npos, states = [], [], [], []
    for b in range(B):
        g = gt[int(offsets[b]):int(offsets[b + 1])]
        state, gi, _ = assign(anchors, g)
        pos = state == 1
        n = int(pos.sum())
        p = cls[b].clamp(1e-4, 1.0 - 1e-4)
        y = torch.zeros(A, nc, dtype=torch.bool)
        if n:
            y[pos, g[gi[pos], 4].long()] = True
        term = torch.where(y, alpha * (1 - p) ** gamma * -torch.log(p), (1 - alpha) * p ** gamma * -torch.log(1 - p))
        term = term * (state != -1)[:, None].to(dt)
        lc.append(term.sum() / max(n, 1))
        if n:
            gg = g[gi[pos]]
            cxg, cyg = gg[:, 0] + 0.5 * (gg[:, 2] - gg[:, 0]), gg[:, 1] + 0.5 * (gg[:, 3] - gg[:, 1])
            wg, hg = (gg[:, 2] - gg[:, 0]).clamp(min=1), (gg[:, 3] - gg[:, 1]).clamp(min=1)
            t = torch.stack([(cyg - cya[pos]) / ha[pos], (cxg - cxa[pos]) / wa[pos], torch.log(hg / ha[pos]), torch.log(wg / wa[pos])], 1)
            d = (t - reg[b][pos]).abs()
            lr.append(torch.where(d <= 1.0 / 9.0, 4.5 * d * d, d - 1.0 / 18.0).mean())
        else:
            lr.append(torch.zeros((), dtype=dt))
        npos.append(n)
        states.append(state)
    return torch.stack(lc).mean(), box_weight * torch.stack(lr).mean(), npos, torch.stack(states)


def loss_and_output_grads(reg, cls, anchors, gt, offsets, dtype, **kw):
    """The losses and dL_regression/dreg, dL_classification/dlogit = dL/dp * p (1 - p), evaluated in `dtype`."""
    r = reg.detach().to(dtype).requires_grad_(True)
    p = cls.detach().to(dtype).requires_grad_(True)
    c, g, npos, state = detection_loss(r, p, anchors, gt, offsets, **kw)
    (c + g).backward()
    pd = p.detach()
    return c.detach(), g.detach(), r.grad, p.grad * pd * (1 - pd), npos, state


def heads_forward(sd, cc: int, nc: int, levels):
    """The heads of detector_ref.eager_forward (its lines 246-254) from the five NCHW feature maps -> (regression,
    classification after the sigmoid)."""
    from stlpose_amd.efficientdet import HEAD_REPEATS
    outs = []
    for head, k in (("regressor", 4), ("classifier", nc)):
        fs = []
        for lv, f in enumerate(levels):
            for i in range(HEAD_REPEATS[cc]):
                f = F.silu(R._bn(sd, f"{head}.bn_list.{lv}.{i}", R._sep(sd, f"{head}.conv_list.{i}", f, norm=False)))
            f = R._sep(sd, f"{head}.header", f, norm=False)
            fs.append(f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, k))
        outs.append(torch.cat(fs, 1))
    return outs[0], torch.sigmoid(outs[1])


def head_state(sd, dtype):
    """The regressor.* / classifier.* entries of sd in `dtype`; the parameters (not the running statistics) require grad."""
    out = {}
    for k, v in sd.items():
        if k.startswith(("regressor.", "classifier.")) and not k.endswith("num_batches_tracked"):
            t = v.detach().cpu().to(dtype).clone()
            out[k] = t if k.endswith(("running_mean", "running_var")) else t.requires_grad_(True)
    return out


def method_yardstick(sd, cc, nc, levels, anchors, gt, offsets, dtype, **kw):
    """detection_loss of heads_forward from the given features, in `dtype` -> (classification, regression, {parameter: grad},
    reg, cls, N_pos)."""
    hs = head_state(sd, dtype)
    reg, cls = heads_forward(hs, cc, nc, [f.detach().cpu().to(dtype) for f in levels])
    c, r, npos, _ = detection_loss(reg, cls, anchors, gt, offsets, **kw)
    (c + r).backward()
    grads = {k: v.grad for k, v in hs.items() if v.requires_grad}
    return c.detach(), r.detach(), grads, reg.detach(), cls.detach(), npos


def rel_err(a, ref) -> float:
    """max|a - ref| / max|ref| (0 / 0 = 0)"""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    den = ref.abs().max().item() if ref.numel() else 0.0
    num = (a - ref).abs().max().item() if ref.numel() else 0.0
    return num / den if den > 0 else num


FLOOR = 1e-6
