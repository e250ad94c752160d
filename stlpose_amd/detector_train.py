"""Fine-tuning the EfficientDet detector on the MI355X: ``EfficientDetBackbone.detection_loss`` (the counterpart of
``loss_dict = self.model(imgs / 255, targets)`` + ``loss.backward()`` in reference ``src/02_train_faster_rcnn.py:189-239``).

The reference has no detection loss for its own EfficientDet; the loss is the published RetinaNet / EfficientDet one (focal
classification + smooth-L1 box regression over IoU-assigned anchors, stl_det_loss in include/stlpose_hip.h), restated in
tests/detector_train_ref.py.  This is the first stage of fine-tuning: the backbone and the BiFPN are frozen and run as the
inference plan's launches, every BN stays on its running statistics (the reference model's ``freeze_bn()``), and the
``regressor.*`` / ``classifier.*`` parameters get gradients.

``HeadTrain`` belongs to one inference plan (one batch size) and lists the training launches once: the heads' forward, then the
backward of every stage that trains, in the reverse of the forward order, one builder per stage, each described where it stands:

    ``_head``         the heads (always)                                               csrc/detector_train.hip
    ``_node``         the last ``train_bifpn`` BiFPN cells (``set_train_bifpn(k)``)          csrc/detector_bifpn.hip
    ``_first_cell``   behind the first cell's nodes (``set_train_bifpn("all")``)
    ``_p5_join``      the gradient of P5 (``set_train_backbone(k)`` / ``set_train_trunk(k)``)
    ``_block``        the last ``train_backbone`` MBConv blocks, the last one first      csrc/detector_mbconv.hip, detector_trunk.hip
    ``_stem``         the stem (``set_train_trunk("all")``)

``_workspaces`` sizes every shared buffer before anything is listed.  The forward is never touched: the inference plan keeps every map a
backward reads (``_Plan.cells`` / ``first_convs`` / ``first_pools`` / ``blocks``) and every pre-activation is recomputed.  The launches produce
gradients of the *folded* weights; ``raw_grads``, ``cell_raw_grads`` and ``block_raw_grads`` carry them to the raw parameters.

A model with ``compute_dtype="f16"`` trains in 16 bit, by the recipe of the pose network's mixed mode: the trunk runs as the 16-bit
inference plan's launches, the heads' forward tensors (every depthwise output d, pre-activation z and swish output t) are f16, the
gradients in flight are bf16, every sum is fp32, and the folded gradients come out in the same fp32 ``grads`` tensors, so
``fold_chain`` and ``raw_grads`` do not change (the contract is stated in include/stlpose_hip.h at stl_det_pointwise16_train).  The
data gradient of a pointwise layer reads a bf16 transposed pack of the folded weight (efficientdet.pack_transposed).  ``"bf16"`` does
not train: its forward error is several times that of f16.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import capi, ops
from .efficientdet import MAX_SIZE, _BiFPN, _device, _is_det_batch, list_dwconv, list_pointwise, resize_meta
from .launch import LaunchList

HEADS = ("regressor", "classifier")
# the backward entry points and workspace queries: fp32 name -> its 16-bit counterpart (the forward ones: efficientdet.list_*)
NAME16 = {"stl_det_pointwise_bwd_slabs": "stl_det_pointwise16_bwd_slabs", "stl_det_dwconv_bwd_parts": "stl_det_dwconv16_bwd_parts",
          "stl_det_pointwise_bwd_weight": "stl_det_pointwise16_bwd_weight", "stl_det_pointwise_bwd_data": "stl_det_pointwise16_bwd_data",
          "stl_det_dwconv_bwd_weight": "stl_det_dwconv16_bwd_weight", "stl_det_dwconv_bwd_data": "stl_det_dwconv16_bwd_data"}
# the first cell's 1x1 layers in the order their weight gradients are listed, and the readers of P5 / P4 / P3 in the order their data gradients join
FIRST_CONVS = ("p5_to_p6", "p3_down_channel", "p4_down_channel", "p5_down_channel", "p4_down_channel_2", "p5_down_channel_2")
P5_READERS, P4_READERS, P3_READERS = ("p5_to_p6", "p5_down_channel", "p5_down_channel_2"), ("p4_down_channel", "p4_down_channel_2"), ("p3_down_channel",)


# ------------------------------------------------------------------------------------------------ targets
def pack_targets(targets, sizes: Sequence[Tuple[int, int]], num_classes: int):
    """The reference's list of target dicts (02_train_faster_rcnn.py:204-209: ``boxes`` [n, 4] x1, y1, x2, y2 in original pixels,
    ``labels`` [n], 1 = the first class) for images of ``sizes`` (height, width) -> (gt float32 [sum n, 5] (x1, y1, x2, y2, class =
    label - 1) on the 512 canvas, scaled by resize_meta's ratios, offsets int32 [B + 1]).  ValueError on anything else."""
    if not isinstance(targets, (list, tuple)) or len(targets) != len(sizes):
        raise ValueError(f"EfficientDet.detection_loss: targets must be a list of {len(sizes)} dicts (one per image)")
    rows, offsets = [], [0]
    for i, (t, (oh, ow)) in enumerate(zip(targets, sizes)):
        if not isinstance(t, dict) or "boxes" not in t or "labels" not in t:
            raise ValueError(f"EfficientDet.detection_loss: targets[{i}] must be a dict with 'boxes' and 'labels'")
        boxes = np.asarray(torch.as_tensor(t["boxes"]).detach().cpu().numpy(), np.float64)
        lab_t = torch.as_tensor(t["labels"]).detach().cpu()
        if lab_t.is_floating_point() or lab_t.dtype == torch.bool:
            raise ValueError(f"EfficientDet.detection_loss: targets[{i}]['labels'] must be integers, got {lab_t.dtype}")
        labels = lab_t.numpy().astype(np.int64)
        if labels.ndim != 1:
            raise ValueError(f"EfficientDet.detection_loss: targets[{i}]['labels'] must be [n], got {labels.shape}")
        n = labels.shape[0]
        if boxes.size == 0 and n == 0:
            boxes = boxes.reshape(0, 4)
        if boxes.ndim != 2 or boxes.shape != (n, 4):
            raise ValueError(f"EfficientDet.detection_loss: targets[{i}]['boxes'] must be [n={n}, 4], got {boxes.shape}")
        if not np.isfinite(boxes).all():
            raise ValueError(f"EfficientDet.detection_loss: targets[{i}]['boxes'] holds a non-finite value")
        if n and (labels.min() < 1 or labels.max() > num_classes):
            raise ValueError(f"EfficientDet.detection_loss: targets[{i}]['labels'] must lie in 1 .. {num_classes}, got "
                             f"{int(labels.min())} .. {int(labels.max())}")
        new_w, new_h = resize_meta(int(oh), int(ow))[:2]
        sx, sy = new_w / ow, new_h / oh
        g = np.concatenate([boxes * np.array([sx, sy, sx, sy]), (labels - 1)[:, None].astype(np.float64)], 1)
        rows.append(g.astype(np.float32))
        offsets.append(offsets[-1] + n)
    return np.concatenate(rows, 0).reshape(-1, 5), np.asarray(offsets, np.int32)


# ------------------------------------------------------------------------------------------------ folded -> raw
def fold_chain(W, b, gamma, mean, var, eps, GW, Gb):
    """Gradients of the folded pointwise layer W' = W s[:, None], b' = b s + beta - mean s, s = gamma / sqrt(var + eps) (frozen
    running statistics), carried to the raw parameters: W, GW [co, ci]; b, gamma, mean, var, Gb [co].  Returns (dW, db, dgamma,
    dbeta).  b None: a conv without bias (b' = beta - mean s); db is None then."""
    r = torch.rsqrt(var + eps)
    s = gamma * r
    ds = (GW * W).sum(1) + Gb * ((b - mean) if b is not None else -mean)
    return GW * s[:, None], None if b is None else Gb * s, ds * r, Gb


def dw_fold_chain(w, gamma, mean, var, eps, Gw, Gb):
    """fold_chain's depthwise counterpart: gradients of the folded depthwise layer w' = w s[:, None, None], b' = beta - mean s (a
    conv without bias under a frozen BN) carried to the raw parameters: w, Gw [c, k, k]; gamma, mean, var, Gb [c].  Returns (dw,
    dgamma, dbeta)."""
    r = torch.rsqrt(var + eps)
    s = gamma * r
    ds = (Gw * w).sum((1, 2)) - Gb * mean
    return Gw * s[:, None, None], ds * r, Gb


def pw_raw_grads(conv, bn, gw, gb):
    """The folded gradients gw [ci, co], gb [co] of the 1x1 ``conv`` under the frozen ``bn`` carried to the raw parameters by
    ``fold_chain``: (conv.weight's [co, ci, 1, 1], conv.bias's or None for a conv without bias, bn.weight's, bn.bias's)."""
    W = conv.weight.detach().reshape(conv.out_channels, conv.in_channels)
    b = None if conv.bias is None else conv.bias.detach()
    dW, db, dgam, dbeta = fold_chain(W, b, bn.weight.detach(), bn.running_mean, bn.running_var, bn.eps, gw.t(), gb)
    return dW[:, :, None, None], db, dgam, dbeta.clone()


# ------------------------------------------------------------------------------------------------ launches
class HeadTrain:
    """The training launches on one inference plan (efficientdet._Plan): the heads' forward (``fwd``) and the backward of every stage
    that trains (``bwd``), the stages in the reverse of the forward order (module docstring)."""

    def __init__(self, m, plan):
        self.B, self.dev, self.c, self.nlayers = plan.B, plan.dev, m.fpn_channels, len(m.regressor.conv_list)
        self.generation = 0   # forwards through these buffers (the stale-backward check of _DetLossFn)
        self.fwd = LaunchList()
        self.bwd = LaunchList(self.fwd.keep)
        self.hdr = {h: [] for h in HEADS}   # the headers' backward descriptors, the very objects `bwd` passes by reference: set_grads sets their dy
        self.h16, self.code, self.adtype = plan.h16, plan.code, plan.adtype   # 16-bit: d / z / t in adtype, ga / gb bf16
        if self.h16:
            m._ensure_transposed()
            self.wbufT, self.layoutT = m._wbufT16, m._layoutT
        self.ncells = m.train_bifpn                    # the trailing BiFPN cells that train with the heads
        self.first = self.ncells == len(plan.cells)    # every cell: the first one's 1x1 layers (Ci = the backbone's channels) and plain pools too
        self.nblocks = m.train_backbone                # the trailing MBConv blocks that train with them
        self.stem = bool(m.train_stem)                 # and the stem (with every block)
        self.specs, nb = m.backbone_net.model.specs, len(plan.blocks)
        self.heads_form = nb - m.final_stage_blocks()  # from this block on: 3 x 3 / 1, the heads' depthwise backward entry points
        self.own_canvas = plan.canvas.data_ptr()
        assert not self.ncells or not self.h16, "the BiFPN cells train in fp32 only"
        assert not self.nblocks or self.first, "the backbone's blocks train with every BiFPN cell only"
        assert not self.stem or self.nblocks == nb, "the stem trains with every block only"
        L, A, nc, dev = m._layout, m.num_anchors_total, m.num_classes, self.dev
        self.reg, self.cls = torch.empty(self.B, A, 4, device=dev), torch.empty(self.B, A, nc, device=dev)
        self._workspaces(plan, nc)
        self.grads, self.cgrads, self.fgrads, self.bgrads = {}, {}, {}, {}   # the folded gradients of the heads, the nodes, the first cell's 1x1 layers, the blocks
        for name, out, k, act in (("regressor", self.reg, 4, 0), ("classifier", self.cls, nc, 2)):
            n, c, aoff = self.nlayers, self.c, 0
            self.grads[name] = dict(pw_w=torch.empty(5, n, c, c, device=dev), pw_b=torch.empty(5, n, c, device=dev),
                                    dw=torch.empty(5, n, 3, 3, c, device=dev), hpw_w=torch.empty(5, c, 9 * k, device=dev),
                                    hpw_b=torch.empty(5, 9 * k, device=dev), hdw=torch.empty(5, 3, 3, c, device=dev))
            for lv, (f, hh) in enumerate(plan.feats):
                self._head(plan, L[name], name, lv, f, hh, out, k, act, dict(img_stride=A * k, row_stride=9 * k, off=aoff * k))
                aoff += hh * hh * 9
        if self.ncells:
            self._levels_join(plan)
            for j in range(len(plan.cells) - 1, len(plan.cells) - self.ncells - 1, -1):
                for node in reversed(_BiFPN.NODES):   # the forward runs them in this tuple's order
                    self._node(plan, L["bifpn"][j][node], j, node)
        if self.first:
            self._first_cell(plan)
        if self.nblocks:
            self.blocks_start = len(self.bwd)   # bwd.calls[blocks_start:] are these launches
            self.block_dy, self.stem_dy = {}, None   # block -> the gradient of its output, after every join; that of the stem's output (train_stem)
            dy = self.gp5 = self._p5_join(plan)
            for i in range(nb - 1, nb - self.nblocks - 1, -1):
                dy = self._block(plan, L["blocks"][i], i, dy, i > nb - self.nblocks or self.stem)
            if self.stem:
                self._stem(plan, L["stem"], dy)

    def _workspaces(self, plan, nc) -> None:
        """Every buffer that launches share, sized from the plan's shapes before anything is listed: the gradients in flight ``ga`` /
        ``gb`` (the largest level), the slab workspaces of the weight gradients (``pw_part``: the largest slabs * (Ci * Co + Co) that is
        listed), the cells' gradient maps (``gmap``) and the scratch the blocks share (``ws``)."""
        B, c, dev, lib = self.B, self.c, self.dev, capi.lib()
        m0 = B * plan.feats[0][1] ** 2
        self.ga, self.gb = (torch.empty(m0 * c, device=dev, dtype=torch.bfloat16 if self.h16 else torch.float32) for _ in range(2))   # reused
        kmax = max(c, 9 * max(4, nc))
        slabs = getattr(lib, self._name("stl_det_pointwise_bwd_slabs"))
        recs = plan.blocks[len(plan.blocks) - self.nblocks:]
        npart = [slabs(m0) * (c * kmax + kmax)]
        if self.first:
            npart += [slabs(r.x.numel() // r.x.shape[3]) * (r.x.shape[3] * c + c) for r in plan.first_convs.values()]
        for r in recs:   # the blocks' project and expand (input resolution) layers
            ci, mid, co = r.inp.shape[3], r.a.shape[3], r.y.shape[3]
            npart += [slabs(r.a.numel() // mid) * (mid * co + co), slabs(r.e.numel() // mid) * (ci * mid + mid) if r.e is not None else 0]
        self.pw_part = torch.empty(max(npart), device=dev)
        self.dw_part = torch.empty(getattr(lib, self._name("stl_det_dwconv_bwd_parts"))(m0) * 9 * c, device=dev)
        if self.ncells:
            # the gradient of every node output of the trainable cells, by the address of the plan's map
            self.gmap = {r.y.data_ptr(): torch.empty_like(r.y) for kept in plan.cells[len(plan.cells) - self.ncells:] for r in kept.values()}
            if self.first:   # and of the first cell's seven input maps (p3_in, p4_in, p5_in, p4_in_2, p5_in_2, p6, p7) and of t
                self.gmap.update({r.y.data_ptr(): torch.empty_like(r.y) for r in [*plan.first_convs.values(), *plan.first_pools]})
            self.written = set()   # the maps whose gradient has its first contribution
            self.hc = [torch.empty_like(f) for f, _ in plan.feats]   # the classifier's gradient of each level (the regressor's goes to gmap)
            self.scale = torch.ones(2, device=dev)                   # the gradients of (regression, classification): _DetLossFn.backward
            self.fuse_ws = torch.empty(lib.stl_det_fuse_bwd_workspace(self.ga.numel()), device=dev)
        if not recs:
            return
        # scratch shared by the blocks, sized for the largest h^2 mid among them: D / du (output resolution); xs / u (output) and z_e
        # (input resolution); dz_e (input resolution); and the small ones
        first, h5 = len(plan.blocks) - len(recs), plan.backbone[2].shape[1]
        dims = [(i, r.inp.shape[1] ** 2 if r.e is not None else 0, r.a.shape[1] ** 2, r.a.shape[3]) for i, r in enumerate(recs, first)]
        flat = lambda n: torch.empty(n, device=dev)   # noqa: E731
        self.ws = ws = SimpleNamespace(
            s1=flat(B * max(hwo * mid for _, _, hwo, mid in dims)),
            s2=flat(B * max(max(hwo, hwe) * mid for _, hwe, hwo, mid in dims)),
            s3=flat(B * max(max(hwe * mid for _, hwe, _, mid in dims), 1)),
            gate_ws=flat(max(lib.stl_det_mbconv_gate_bwd_workspace(B, hwo, mid) for _, _, hwo, mid in dims)),
            act_ws=flat(max(lib.stl_det_mbconv_act_bwd_workspace(B, hwo, mid) for _, _, hwo, mid in dims)),
            se_ws=flat(max(lib.stl_det_se_bwd_workspace(B, mid, self.specs[i]["se"]) for i, _, _, mid in dims)),
            asum=flat(B * max(d[3] for d in dims)), dgate=flat(B * max(d[3] for d in dims)), dpool=flat(B * max(d[3] for d in dims)),   # [B, mid]
            dwb_part=flat(lib.stl_det_dwconv_bwd_parts(B * h5 * h5) * 9 * max(mid for i, _, _, mid in dims if i >= self.heads_form)),
            ks_part=flat(max([lib.stl_det_dwconv_bwd_ks_parts(B * hwo) * self.specs[i]["k"] ** 2 * mid
                              for i, _, hwo, mid in dims if i < self.heads_form] + [1])))
        self.bwd.keep_alive(*vars(ws).values())

    def _name(self, name: str) -> str:
        return NAME16[name] if self.h16 else name

    def _pw_desc(self, plan, pk, x, dy, dx, gw, gb, hw, ci, co, img_stride=None, row_stride=None, off=0):
        """The backward descriptor of the pointwise layer packed as pk = (w, bias, Kp, Np), x [B hw, ci], dy [B hw, co], for
        stl_det_pointwise_bwd_weight (x, gw, gb, and the slab workspace with them), stl_det_pointwise_bwd_data (dx [B hw, ci] = dy W'^T,
        and the folded weight with it) or both; the strides and the offset place dy's rows inside a larger output.  dy None: a header,
        whose dy (dreg / dlogit, fp32) set_grads fills in.  Keeps the owners alive."""
        w, _, kp, np_ = pk
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rest = (ptr(dy), ptr(dx), ptr(gw), ptr(gb), None if gw is None else self.pw_part.data_ptr(), self.B * hw,
                hw * co if img_stride is None else img_stride, co if row_stride is None else row_stride, off, hw, ci, co)
        if self.h16:
            wt, kt, nt = self.layoutT[w]
            p = capi.DetPointwise16Bwd(ptr(x), self.wbufT[wt:].data_ptr(), *rest, kt, nt, self.code, 1 if dy is None else 0, 0)
        else:
            p = capi.DetPointwiseBwd(ptr(x), None if dx is None else plan.wbuf[w:].data_ptr(), *rest, kp, np_, 0)
        self.bwd.keep_alive(x, dy, dx, gw, gb)   # the descriptor holds their addresses
        return p

    def _dw_bwd(self, x, dy, w, gw, z, dx, h):
        """Weight gradient of one depthwise layer and, with dx, its data gradient times swish'(z) of the layer below."""
        code = (self.code,) if self.h16 else ()   # the 16-bit entry points take the forward tensors' type: first / last argument
        self.bwd.add(self._name("stl_det_dwconv_bwd_weight"), *code, x, dy, self.dw_part, gw, self.B, h, h, self.c)
        if dx is not None:
            self.bwd.add(self._name("stl_det_dwconv_bwd_data"), dy, w, z, dx, self.B, h, h, self.c, *code)

    def _head(self, plan, lay, name, lv, f, hh, out, k, act, strides) -> None:
        """One (head, level).  Its forward runs the head with the inference kernels -- ``reg`` and ``cls`` equal the inference plan's
        bit for bit -- and keeps what the backward needs: every depthwise output, and the pre-activation ``z`` of every swish, written
        by the pointwise launch that applies it (stl_det_pointwise_train).  Its backward walks from the header down through
        csrc/detector_train.hip and produces gradients of the *folded* weights W' = W s, b' = b s + t (s, t the frozen BN's scale and
        shift) per level; ``fold_chain`` carries them to W, b, gamma and beta in a few elementwise torch ops, and the weights shared
        by the five levels sum their five contributions.  The first depthwise layer of a (head, level) reads a frozen feature map:
        no data gradient is computed for it.  Where cells train, it also computes its data gradient (stl_det_dwconv_bwd_data without
        z): the regressor's into the level's gradient map, the classifier's into ``hc``."""
        B, c, n, g, hw = self.B, self.c, self.nlayers, self.grads[name], hh * hh
        buf = lambda: torch.empty(B, hh, hh, c, device=self.dev, dtype=self.adtype)   # noqa: E731
        t, d, z = [f], [], []
        for i in range(n):
            d.append(buf()), z.append(buf()), t.append(buf())
            list_dwconv(self.fwd, self.code, t[i], plan._w(lay["dw"][i]), None, d[i], B, hh, c, 3, 1, 0)
            list_pointwise(self.fwd, self.code, plan.pw_fields(d[i], t[i + 1], hw, c, c, lay["pw"][lv][i], 1), False, z=z[i])
        dh = buf()
        list_dwconv(self.fwd, self.code, t[n], plan._w(lay["hdw"]), None, dh, B, hh, c, 3, 1, 0)
        list_pointwise(self.fwd, self.code, plan.pw_fields(dh, out, hw, c, 9 * k, lay["hpw"], act, **strides), True)
        self.fwd.keep_alive(*d, *t, dh)   # the pointwise descriptors hold their addresses
        # backward, from the header down; ga / gb alternate as the gradient of a depthwise / a pointwise output
        weight, data = self._name("stl_det_pointwise_bwd_weight"), self._name("stl_det_pointwise_bwd_data")
        p = self._pw_desc(plan, lay["hpw"], dh, None, self.ga, g["hpw_w"][lv], g["hpw_b"][lv], hw, c, 9 * k, **strides)
        self.hdr[name].append(p)
        self.bwd.add(weight, p)
        self.bwd.add(data, p)
        self._dw_bwd(t[n], self.ga, plan._w(lay["hdw"]), g["hdw"][lv], z[n - 1], self.gb, hh)
        for i in range(n - 1, -1, -1):
            p = self._pw_desc(plan, lay["pw"][lv][i], d[i], self.gb, self.ga, g["pw_w"][lv, i], g["pw_b"][lv, i], hw, c, c)
            self.bwd.add(weight, p)
            self.bwd.add(data, p)
            dx0 = None if not self.ncells else (self.gmap[f.data_ptr()] if name == "regressor" else self.hc[lv])
            self._dw_bwd(t[i], self.ga, plan._w(lay["dw"][i]), g["dw"][lv, i], z[i - 1] if i else None, self.gb if i else dx0, hh)

    def _levels_join(self, plan) -> None:
        """Behind the heads where cells train: the two heads' gradients of a level are added regressor first, each times the gradient
        of its own loss (stl_det_grad_add reads the two scalars on the device)."""
        for lv, (f, _) in enumerate(plan.feats):
            g = self.gmap[f.data_ptr()]
            self.bwd.add("stl_det_grad_add", g, self.hc[lv], self.scale, self.scale[1:], g, g.numel())
            self.written.add(f.data_ptr())

    def _node(self, plan, lay, j, node) -> None:
        """One node of a trainable cell: ``model.set_train_bifpn(k)`` (1 <= k <= cells - 1, or "all": ``_first_cell``) trains the last k
        BiFPN cells with the heads, fp32 only.  The forward is not touched: the inference plan keeps every map (``_Plan.cells``), and
        the backward recomputes each node's pre-activation from them.  The cells run in reverse, the nodes of a cell in the reverse
        of the forward order.  Every consumer of a map comes later in the forward order, so a map's gradient is complete when its
        node is reached; the first contribution writes, the later ones accumulate, in that fixed order.  Per node: the pointwise
        layer's weight and data gradient (x = d), the depthwise layer's weight gradient (x = f) and data gradient, then
        stl_det_fuse_bwd (csrc/detector_bifpn.hip), whose destinations are null for the frozen inputs of the first trainable cell.
        ``cell_raw_grads`` carries the folded gradients to the raw parameters: ``fold_chain`` for the pointwise layer and its BN,
        ``fusion_weight_grads`` for ``p*_w1`` / ``p*_w2``."""
        r, c, dev = plan.cells[j][node], self.c, self.dev
        assert r.y.data_ptr() in self.written, (j, node)
        h = r.y.shape[1]
        g = self.cgrads[j, node] = dict(pw_w=torch.empty(c, c, device=dev), pw_b=torch.empty(c, device=dev),
                                        dw=torch.empty(3, 3, c, device=dev), what=torch.zeros(3, device=dev))
        p = self._pw_desc(plan, lay[1], r.d, self.gmap[r.y.data_ptr()], self.ga, g["pw_w"], g["pw_b"], h * h, c, c)
        self.bwd.add("stl_det_pointwise_bwd_weight", p)
        self.bwd.add("stl_det_pointwise_bwd_data", p)
        self._dw_bwd(r.f, self.ga, plan._w(lay[0]), g["dw"], None, self.gb, h)
        fb = capi.DetFuseBwd()
        for i, t in enumerate(r.terms):   # a term outside gmap is an input of the first trainable cell: frozen
            dst = self.gmap.get(t.data_ptr())
            if dst is not None:
                fb.dx[i], fb.accumulate[i] = dst.data_ptr(), int(t.data_ptr() in self.written)
                self.written.add(t.data_ptr())
        self.bwd.keep_alive(r.f, r.d, r.y, *r.terms)   # the descriptors hold their addresses
        self.bwd.add("stl_det_fuse_bwd", r.desc, self.gb, fb, self.fuse_ws, g["what"])

    def _first_cell(self, plan) -> None:
        """``model.set_train_bifpn("all")`` trains the first cell too, so everything behind the frozen backbone.  Its eight nodes run
        through ``_node``; their inputs are the seven maps the cell makes from P3 / P4 / P5 (``p3_in``, ``p4_in``, ``p5_in``, the second
        ``p4_in`` / ``p5_in`` of the down path, ``p6``, ``p7``), which get gradient maps like any node output.  Behind the nodes:
        stl_det_pool_bwd (csrc/detector_bifpn.hip) of ``p6 -> p7``, adding to the gradient of ``p6``, which is complete then, then of
        ``t -> p6`` (``t`` the output of ``p5_to_p6``'s conv and BN), then the weight gradients of the six 1x1 layers
        (stl_det_pointwise_bwd_weight with x = the backbone map: ``p5_to_p6``, the three ``*_down_channel``, the two
        ``*_down_channel_2``; ``_Plan.first_pools`` / ``first_convs``).  No data gradient is computed for P3 / P4 / P5 here (``_p5_join``,
        ``_block``: where blocks train).  ``fold_chain`` carries each folded pair to the conv's weight and bias and the BN's."""
        c, dev = self.c, self.dev
        for r in reversed(plan.first_pools):
            assert r.y.data_ptr() in self.written, "a pooled map of the first cell without a gradient"
            self.bwd.keep_alive(r.x, r.y)
            self.bwd.add("stl_det_pool_bwd", r.desc, self.gmap[r.y.data_ptr()], self.gmap[r.x.data_ptr()], int(r.x.data_ptr() in self.written))
            self.written.add(r.x.data_ptr())
        assert sorted(FIRST_CONVS) == sorted(plan.first_convs)
        for key in FIRST_CONVS:
            r = plan.first_convs[key]
            assert r.y.data_ptr() in self.written, key
            ci, hw = r.x.shape[3], r.x.shape[1] * r.x.shape[2]
            g = self.fgrads[key] = dict(pw_w=torch.empty(ci, c, device=dev), pw_b=torch.empty(c, device=dev))
            self.bwd.add("stl_det_pointwise_bwd_weight",
                         self._pw_desc(plan, r.pk, r.x, self.gmap[r.y.data_ptr()], None, g["pw_w"], g["pw_b"], hw, ci, c))

    def _first_conv_bwd_data(self, plan, key, x) -> torch.Tensor:
        """The data gradient of the first cell's 1x1 layer ``key``, which reads the backbone map x, into a buffer of its own."""
        r = plan.first_convs[key]
        assert r.x is x, key
        t = torch.empty_like(x)
        self.bwd.add("stl_det_pointwise_bwd_data",
                     self._pw_desc(plan, r.pk, None, self.gmap[r.y.data_ptr()], t, None, None, x.shape[1] * x.shape[2], x.shape[3], self.c))
        return t

    def _p5_join(self, plan) -> torch.Tensor:
        """``model.set_train_backbone(k)`` (needs "all"; fp32) trains the last k MBConv blocks of the backbone's final stage too (block 15
        of D0, blocks 24 / 25 of D3: 3x3 stride-1 depthwise layers).  Behind the cells' launches: stl_det_pointwise_bwd_data of
        ``p5_to_p6``, ``p5_down_channel`` and ``p5_down_channel_2`` into a buffer each, joined in that order by stl_det_grad_add -- the
        gradient of P5, which this returns."""
        p5 = plan.backbone[2]
        assert plan.blocks[-1].y is p5
        parts = [self._first_conv_bwd_data(plan, key, p5) for key in P5_READERS]
        for t in parts[1:]:
            self.bwd.add("stl_det_grad_add", parts[0], t, None, None, parts[0], parts[0].numel())
        return parts[0]

    def _block_dw_bwd(self, i, kind, hi, *ptrs) -> None:
        """Lists the depthwise weight gradient (kind "weight": x, dy, gw) or data gradient ("data": dy, w, z, dx) of block i on its hi x hi
        input: a block of the final stage through the heads' entry points, one in front of it through stl_det_dwconv_bwd_weight_ks /
        _data_ks (csrc/detector_trunk.hip: k 3 / 5, s 1 / 2 under TF "same" padding).  The two sum in different orders: the split is fixed."""
        b, old = self.specs[i], i >= self.heads_form
        assert not old or (b["k"] == 3 and b["s"] == 1 and b["e"] != 1), i
        if kind == "weight":
            ptrs = (*ptrs[:2], self.ws.dwb_part if old else self.ws.ks_part, ptrs[2])
        self.bwd.add(f"stl_det_dwconv_bwd_{kind}" + ("" if old else "_ks"), *ptrs, self.B, hi, hi, b["mid"], *(() if old else (b["k"], b["s"])))

    def _block(self, plan, lay, i, dy, need_dx):
        """MBConv block i from dy, the gradient of its output; need_dx: the block (or the stem) in front trains too, and the gradient
        of this block's input is returned.  The forward is the inference forward (no drop-connect, BN on running statistics);
        ``_Plan.blocks`` keeps each block's input, expand output e, depthwise output a, gate g and output.  With the folded weights: D =
        dy Wp'^T (stl_det_pointwise_bwd_data); stl_det_mbconv_gate_bwd (csrc/detector_mbconv.hip: xs = a g, sum a, sum D a); the
        projection's weight gradient with x = xs; stl_det_se_bwd (dpool and the four SE gradients); the depthwise pre-activation u
        recomputed by stl_det_dwconv at act 0; stl_det_mbconv_act_bwd (du = (D g + dpool / HW) swish'(u) over D, and the folded BN's
        bias gradient); stl_det_dwconv_bwd_weight (x = e); the expand layer's pre-activation recomputed by stl_det_pointwise at act 0;
        stl_det_dwconv_bwd_data (times swish' of it); the expand layer's weight gradient (x = the block input); and, where the block
        in front trains too, its data gradient plus dy through the skip.  ``block_raw_grads`` carries the folded gradients to the raw
        parameters (``fold_chain`` without a conv bias, ``dw_fold_chain``).

        ``model.set_train_trunk(k)`` reaches further back: the last k blocks of the whole backbone, ``"all"`` the stem too.  The final
        stage's blocks keep the launches above; a block in front of it runs the same sequence with the k x k / s depthwise entry
        points (``_block_dw_bwd``), the projection, gate, SE and act steps at the block's output resolution, the expand recompute, the
        depthwise data gradient and the expand gradients at its input resolution.  A block without an expand layer (e = 1) has no
        ``exp_w`` / ``exp_b``: its depthwise layer reads the block input, and stl_det_dwconv_bwd_data_ks without z is the input's
        gradient.  The gradient of a block's input is joined in a fixed order: the block's own data gradient, dy through the skip,
        then -- where the input is P4 / P3, the inputs of the last two stride-2 blocks -- stl_det_pointwise_bwd_data of
        ``p4_down_channel`` and ``p4_down_channel_2`` / of ``p3_down_channel``, each into a buffer of its own and added by
        stl_det_grad_add.  ``tr.block_dy[i]`` keeps the joined gradient of block i's output."""
        B, dev, ws, b, r = self.B, self.dev, self.ws, self.specs[i], plan.blocks[i]
        ci, mid, co, cs, k, s = b["ci"], b["mid"], b["co"], b["se"], b["k"], b["s"]
        hi, ho, hwi, hwo = r.inp.shape[1], r.a.shape[1], r.inp.shape[1] ** 2, r.a.shape[1] ** 2
        assert dy.shape == r.y.shape and (r.e is None) == (b["e"] == 1) and ho == (hi + s - 1) // s, i
        self.block_dy[i] = dy
        g = self.bgrads[i] = dict(exp_w=torch.empty(ci, mid, device=dev), exp_b=torch.empty(mid, device=dev)) if r.e is not None else {}
        g.update(dw=torch.empty(k, k, mid, device=dev), dw_b=torch.empty(mid, device=dev), se_w1=torch.empty(cs, mid, device=dev),
                 se_b1=torch.empty(cs, device=dev), se_w2=torch.empty(mid, cs, device=dev), se_b2=torch.empty(mid, device=dev),
                 proj_w=torch.empty(mid, co, device=dev), proj_b=torch.empty(co, device=dev))
        self.bwd.keep_alive(*r, *g.values())
        wd, bd = plan._w(lay["dw"][0]), plan._w(lay["dw"][1])
        xd = r.inp if r.e is None else r.e   # what the depthwise layer reads
        # the projection: D = dy Wp'^T; xs = a g, asum, dgate; dWp', dbp' with x = xs
        self.bwd.add("stl_det_pointwise_bwd_data", self._pw_desc(plan, lay["project"], None, dy, ws.s1, None, None, hwo, mid, co))
        self.bwd.add("stl_det_mbconv_gate_bwd", r.a, ws.s1, r.gate, ws.s2, ws.gate_ws, ws.asum, ws.dgate, B, hwo, mid)
        self.bwd.add("stl_det_pointwise_bwd_weight", self._pw_desc(plan, lay["project"], ws.s2, dy, None, g["proj_w"], g["proj_b"], hwo, mid, co))
        # the gate: dpool and the SE gradients
        self.bwd.add("stl_det_se_bwd", ws.asum, ws.dgate, r.gate, B, hwo, mid, cs, *[plan._w(o) for o in lay["se"]], ws.se_ws, ws.dpool,
                     g["se_w1"], g["se_b1"], g["se_w2"], g["se_b2"])
        # the depthwise layer: u recomputed by the forward's launch without the activation; du overwrites D; db_d'; dw_d'
        list_dwconv(self.bwd, 0, xd, wd, bd, ws.s2, B, hi, mid, k, s, 0)
        self.bwd.add("stl_det_mbconv_act_bwd", ws.s1, ws.s2, r.gate, ws.dpool, ws.s1, ws.act_ws, g["dw_b"], B, hwo, mid)
        self._block_dw_bwd(i, "weight", hi, xd, ws.s1, g["dw"])
        dx = torch.empty_like(r.inp) if need_dx else None
        if r.e is not None:
            # the expand layer: its pre-activation z_e recomputed the same way, dz_e = dwconv^T(du) swish'(z_e); dWe', dbe'
            list_pointwise(self.bwd, 0, plan.pw_fields(r.inp, ws.s2, hwi, ci, mid, lay["expand"], 0), False)
            self._block_dw_bwd(i, "data", hi, ws.s1, wd, ws.s2, ws.s3)
            self.bwd.add("stl_det_pointwise_bwd_weight", self._pw_desc(plan, lay["expand"], r.inp, ws.s3, None, g["exp_w"], g["exp_b"], hwi, ci, mid))
            if need_dx:
                self.bwd.add("stl_det_pointwise_bwd_data", self._pw_desc(plan, lay["expand"], None, ws.s3, dx, None, None, hwi, ci, mid))
        elif need_dx:   # no expand layer: the depthwise layer reads the block input, its data gradient is the input's
            self._block_dw_bwd(i, "data", hi, ws.s1, wd, None, dx)
        if need_dx:
            # joined in this order: the block's own data gradient, dy through the skip, then -- where the input is P4 / P3 -- the
            # data gradients of the first cell's 1x1 layers that read it: p4_down_channel, p4_down_channel_2 / p3_down_channel
            if b["skip"]:
                self.bwd.add("stl_det_grad_add", dx, dy, None, None, dx, dx.numel())
            p3, p4, _ = plan.backbone
            for key in P4_READERS if r.inp is p4 else P3_READERS if r.inp is p3 else ():
                self.bwd.add("stl_det_grad_add", dx, self._first_conv_bwd_data(plan, key, r.inp), None, None, dx, dx.numel())
        return dx

    def _stem(self, plan, lay, dy) -> None:
        """With the stem, block 0 also produces its input's gradient (``tr.stem_dy``, that of the stem's output) and stl_det_stem_bwd
        follows (the pre-activation recomputed from the canvas the forward read; no image gradient); its ``[3][3][3][Co]`` gradient is
        permuted to ``[Co, 3, 3, 3]`` and folded through ``_bn0`` as a conv without bias (``block_raw_grads``)."""
        assert dy.shape == plan.blocks[0].inp.shape
        self.stem_dy = dy
        S, ho, co, dev = plan.canvas.shape[1], dy.shape[1], dy.shape[3], self.dev
        self.sgrads = dict(w=torch.empty(3, 3, 3, co, device=dev), b=torch.empty(co, device=dev))
        stem_part = torch.empty(capi.lib().stl_det_stem_bwd_parts(self.B * ho * ho) * 28 * co, device=dev)
        # the canvas the forward read: the plan's own, or the batch's (set_canvas before each backward)
        self.canvas_arg = ctypes.c_void_p(plan.canvas.data_ptr())
        self.bwd.keep_alive(plan.canvas, dy, stem_part, *self.sgrads.values())
        self.bwd.add("stl_det_stem_bwd", self.canvas_arg, plan._w(lay[0]), plan._w(lay[1]), dy, stem_part, self.sgrads["w"],
                     self.sgrads["b"], self.B, S, S, co)

    def set_canvas(self, canvas) -> None:
        """The canvas the forward about to be differentiated read (None: the plan's own); the caller keeps it alive until the backward."""
        if self.stem:
            self.canvas_arg.value = self.own_canvas if canvas is None else canvas.data_ptr()

    def set_grads(self, dreg: torch.Tensor, dlogit: torch.Tensor) -> None:
        self.dreg, self.dlogit = dreg, dlogit
        for name, t in (("regressor", dreg), ("classifier", dlogit)):
            for p in self.hdr[name]:
                p.dy = t.data_ptr()

    def forward(self, stream: int) -> None:
        self.generation += 1
        self.fwd.run(stream)

    def backward(self, stream: int) -> None:
        self.bwd.run(stream)


# ------------------------------------------------------------------------------------------------ autograd
def head_parameters(m) -> List[Tuple[str, torch.nn.Parameter]]:
    return [(f"{h}.{n}", p) for h in HEADS for n, p in getattr(m, h).named_parameters()]


def trainable_parameters(m) -> List[Tuple[str, torch.nn.Parameter]]:
    """What detection_loss differentiates: with ``m.train_stem`` the stem's conv weight and its BN's weight and bias, then the parameters
    of the last ``m.train_backbone`` MBConv blocks in state_dict order (expand conv and BN -- not in a block without an expand layer --,
    depthwise conv and BN, the two SE convs, project conv and BN), then those of the last ``m.train_bifpn`` BiFPN cells
    in state_dict order (after ``set_train_bifpn("all")`` every cell's, the first cell's 24 conv and BN tensors among them), then
    head_parameters(m)."""
    kb = getattr(m, "train_backbone", 0)   # (the trainer's tests pass models that have the heads only)
    allb = m.backbone_net.model._blocks if kb else ()
    blocks = [(f"backbone_net.model._blocks.{i}.{name}", p) for i in range(len(allb) - kb, len(allb)) for name, p in allb[i].named_parameters()]
    if getattr(m, "train_stem", False):   # set_train_trunk("all"): the stem's three tensors first (a block without an expand layer has 10, the others 13)
        net = m.backbone_net.model
        blocks = [("backbone_net.model._conv_stem.conv.weight", net._conv_stem.conv.weight), ("backbone_net.model._bn0.weight", net._bn0.weight),
                  ("backbone_net.model._bn0.bias", net._bn0.bias)] + blocks
    k = getattr(m, "train_bifpn", 0)
    n = len(m.bifpn) if k else 0
    cells = [(f"bifpn.{j}.{name}", p) for j in range(n - k, n) for name, p in m.bifpn[j].named_parameters()]
    return blocks + cells + head_parameters(m)


def fusion_weight_grads(p: torch.Tensor, dwhat: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """The gradient of a node's raw fusion weights p [n] from that of the normalised w^_i = relu(p_i) / (sum_j relu(p_j) + eps):
    dL/dp_j = dw^_j / S - sum_i dw^_i relu(p_i) / S^2 with S = sum relu(p) + eps where p_j > 0, and 0 where p_j <= 0."""
    r = torch.relu(p)
    S = r.sum() + eps
    return torch.where(p > 0, dwhat / S - (dwhat * r).sum() / (S * S), torch.zeros_like(p))


def cell_raw_grads(m, tr: HeadTrain) -> Dict[str, torch.Tensor]:
    """{parameter name: gradient} of every parameter of the trainable BiFPN cells from the folded per-node gradients of tr."""
    out = {}
    for (j, node), g in tr.cgrads.items():
        sep, pre = getattr(m.bifpn[j], node), f"bifpn.{j}.{node}."
        out[pre + "depthwise_conv.conv.weight"] = g["dw"].permute(2, 0, 1)[:, None]
        (out[pre + "pointwise_conv.conv.weight"], out[pre + "pointwise_conv.conv.bias"], out[pre + "bn.weight"],
         out[pre + "bn.bias"]) = pw_raw_grads(sep.pointwise_conv.conv, sep.bn, g["pw_w"], g["pw_b"])
        wname = dict(zip(_BiFPN.NODES, _BiFPN.WEIGHTS))[node][0]
        p = getattr(m.bifpn[j], wname).detach()
        out[f"bifpn.{j}.{wname}"] = fusion_weight_grads(p, g["what"][:p.numel()])
    for key, g in tr.fgrads.items():   # the first cell's 1x1 layers: Sequential(conv, BN[, pool])
        seq, pre = getattr(m.bifpn[0], key), f"bifpn.0.{key}."
        out[pre + "0.conv.weight"], out[pre + "0.conv.bias"], out[pre + "1.weight"], out[pre + "1.bias"] = \
            pw_raw_grads(seq[0].conv, seq[1], g["pw_w"], g["pw_b"])
    return out


def block_raw_grads(m, tr: HeadTrain) -> Dict[str, torch.Tensor]:
    """{parameter name: gradient} of every parameter of the trainable MBConv blocks from the folded per-block gradients of tr: the
    two pointwise layers by ``fold_chain`` (convs without bias), the depthwise layer by ``dw_fold_chain``, the SE convs as they are."""
    out = {}
    for i, g in tr.bgrads.items():
        blk, pre = m.backbone_net.model._blocks[i], f"backbone_net.model._blocks.{i}."
        layers = [("_expand_conv", "_bn0", g["exp_w"], g["exp_b"])] if "exp_w" in g else []   # (a block without an expand layer)
        for conv, bn, gw, gb in layers + [("_project_conv", "_bn2", g["proj_w"], g["proj_b"])]:
            out[pre + conv + ".conv.weight"], _, out[pre + bn + ".weight"], out[pre + bn + ".bias"] = \
                pw_raw_grads(getattr(blk, conv).conv, getattr(blk, bn), gw, gb)
        n = blk._bn1
        dw, dgam, dbeta = dw_fold_chain(blk._depthwise_conv.conv.weight.detach()[:, 0], n.weight.detach(), n.running_mean, n.running_var,
                                        n.eps, g["dw"].permute(2, 0, 1), g["dw_b"])
        out[pre + "_depthwise_conv.conv.weight"] = dw[:, None]
        out[pre + "_bn1.weight"], out[pre + "_bn1.bias"] = dgam, dbeta.clone()
        out[pre + "_se_reduce.conv.weight"], out[pre + "_se_reduce.conv.bias"] = g["se_w1"][:, :, None, None].clone(), g["se_b1"].clone()
        out[pre + "_se_expand.conv.weight"], out[pre + "_se_expand.conv.bias"] = g["se_w2"][:, :, None, None].clone(), g["se_b2"].clone()
    if tr.stem:   # the stem: [3][3][3][Co] -> [Co, 3, 3, 3], folded through _bn0 as a conv without bias
        net, pre, g = m.backbone_net.model, "backbone_net.model.", tr.sgrads
        W, n = net._conv_stem.conv.weight.detach(), net._bn0
        dW, _, dgam, dbeta = fold_chain(W.reshape(W.shape[0], -1), None, n.weight.detach(), n.running_mean, n.running_var, n.eps,
                                        g["w"].permute(3, 2, 0, 1).reshape(W.shape[0], -1), g["b"])
        out[pre + "_conv_stem.conv.weight"] = dW.reshape(W.shape)
        out[pre + "_bn0.weight"], out[pre + "_bn0.bias"] = dgam, dbeta.clone()
    return out


def raw_grads(m, tr: HeadTrain) -> Dict[str, torch.Tensor]:
    """{parameter name: gradient} of every regressor.* / classifier.* parameter from the folded per-level gradients of tr."""
    out = {}
    for h in HEADS:
        hd, g = getattr(m, h), tr.grads[h]
        for i, cv in enumerate(hd.conv_list):
            pre, pw = f"{h}.conv_list.{i}.", cv.pointwise_conv.conv
            out[pre + "depthwise_conv.conv.weight"] = g["dw"][:, i].sum(0).permute(2, 0, 1)[:, None]
            dW, db = torch.zeros_like(pw.weight), torch.zeros_like(pw.bias)
            for lv in range(5):   # the conv is shared by the five levels, each with a BN of its own
                a, bb, out[f"{h}.bn_list.{lv}.{i}.weight"], out[f"{h}.bn_list.{lv}.{i}.bias"] = \
                    pw_raw_grads(pw, hd.bn_list[lv][i], g["pw_w"][lv, i], g["pw_b"][lv, i])
                dW, db = dW + a, db + bb
            out[pre + "pointwise_conv.conv.weight"], out[pre + "pointwise_conv.conv.bias"] = dW, db
        out[f"{h}.header.depthwise_conv.conv.weight"] = g["hdw"].sum(0).permute(2, 0, 1)[:, None]
        out[f"{h}.header.pointwise_conv.conv.weight"] = g["hpw_w"].sum(0).t()[:, :, None, None]
        out[f"{h}.header.pointwise_conv.conv.bias"] = g["hpw_b"].sum(0)
    return out


class _DetLossFn(torch.autograd.Function):
    """(classification, regression) as functions of trainable_parameters: forward hands out the losses stl_det_loss computed,
    backward runs the backward launches (the heads', then the trainable cells') and the folded-to-raw chain."""

    @staticmethod
    def forward(ctx, m, tr, names, losses, *params):
        ctx.m, ctx.tr, ctx.names, ctx.generation = m, tr, names, tr.generation
        return losses[0].clone(), losses[1].clone()

    @staticmethod
    def backward(ctx, gc, gr):
        tr = ctx.tr
        if ctx.generation != tr.generation:
            raise RuntimeError(
                "stlpose_amd.EfficientDetBackbone: backward through a stale forward -- the plan for this batch size ran "
                f"detection_loss #{tr.generation} after the one (#{ctx.generation}) being differentiated, and its activations "
                "were overwritten (the reference's autograd keeps one set per call; this engine keeps one per plan).  Call "
                "backward before the next detection_loss of the same batch size.")
        with torch.no_grad():
            if tr.ncells:   # the cells' gradients are linear in both: stl_det_grad_add scales the heads' two contributions
                tr.scale.copy_(torch.stack([gr, gc]))
            tr.backward(ops._st())
            grads = raw_grads(ctx.m, tr)
            scale = {"regressor": gr, "classifier": gc}   # dreg / dlogit are the gradients of the regression / classification loss
            out = [grads[n].contiguous() * scale[n.split(".", 1)[0]] for n in ctx.names if n.startswith(HEADS)]
            if tr.ncells:
                cells = cell_raw_grads(ctx.m, tr)
                out = [cells[n].contiguous() for n in ctx.names if n.startswith("bifpn.")] + out
            if tr.nblocks:
                blocks = block_raw_grads(ctx.m, tr)
                out = [blocks[n].contiguous() for n in ctx.names if n.startswith("backbone_net.")] + out
        return (None, None, None, None, *out)


def detection_loss(m, inputs, targets, alpha: float = 0.25, gamma: float = 2.0, box_weight: float = 50.0) -> Dict[str, torch.Tensor]:
    """EfficientDetBackbone.detection_loss (documented there)."""
    if m.compute_dtype not in ("fp32", "f16"):
        raise NotImplementedError(f"EfficientDet.detection_loss: compute_dtype {m.compute_dtype!r}; the heads train in \"fp32\" or "
                                  "\"f16\" (f16 forward, bf16 gradients)")
    if m.train_bifpn and m.compute_dtype != "fp32":
        raise NotImplementedError(f"EfficientDet.detection_loss: compute_dtype {m.compute_dtype!r} with train_bifpn = {m.train_bifpn}; "
                                  "the BiFPN cells train in \"fp32\" only (16-bit models train their heads: set_train_bifpn(0))")
    st = ops._st()
    if _is_det_batch(inputs):   # det_data.DetBatch: the canvas and the ground-truth table are on the device already
        if targets is not None:
            raise ValueError("EfficientDet.detection_loss: a DetBatch carries its targets (gt, offsets); pass no targets with it")
        dev = _device(inputs.canvas.device)
        p, canvas, keep = m.plan(len(inputs), dev), inputs.canvas, inputs
        gt_dev, offsets_dev = inputs.gt, inputs.offsets
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        srcs = m._float_sources(inputs, dev)
        gt, offsets = pack_targets(targets, [(int(s.shape[1]), int(s.shape[2])) for s in srcs], m.num_classes)
        with torch.no_grad():
            p, _, keep = m._preprocess(srcs, 1, dev)
        canvas, gt_dev, offsets_dev = None, torch.from_numpy(gt).to(dev), torch.from_numpy(offsets).to(dev)
    with torch.no_grad():
        if p.train is None or p.train.ncells != m.train_bifpn or p.train.nblocks != m.train_backbone or p.train.stem != m.train_stem:
            p.train = HeadTrain(m, p)
        tr = p.train
        tr.set_canvas(canvas)
        p.run(st, upto=p.head_start, canvas=canvas)
        tr.forward(st)
        p._inflight = keep
        if tr.h16 and not bool((torch.isfinite(tr.reg).all() & torch.isfinite(tr.cls).all()).item()):
            raise FloatingPointError("EfficientDet.detection_loss: non-finite head outputs in compute_dtype='f16': activations left "
                                     "f16's range (largest finite value 65504); fine-tune the detector with compute_dtype=\"fp32\"")
        losses, dreg, dlogit, npos = torch.ops.stlpose.det_loss(tr.reg, tr.cls, m._anchor_dev, gt_dev, offsets_dev, float(alpha),
                                                                float(gamma), float(box_weight))
        tr.set_grads(dreg, dlogit)
        tr.npos = npos
    named = trainable_parameters(m)
    c, r = _DetLossFn.apply(m, tr, [n for n, _ in named], losses, *[q for _, q in named])
    return {"classification": c, "regression": r}
