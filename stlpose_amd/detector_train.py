"""Fine-tuning the EfficientDet heads on the MI355X: ``EfficientDetBackbone.detection_loss`` (the counterpart of
``loss_dict = self.model(imgs / 255, targets)`` + ``loss.backward()`` in reference ``src/02_train_faster_rcnn.py:189-239``).

The reference has no detection loss for its own EfficientDet; the loss is the published RetinaNet / EfficientDet one (focal
classification + smooth-L1 box regression over IoU-assigned anchors, stl_det_loss in include/stlpose_hip.h), restated in
tests/detector_train_ref.py.  This is the first stage of fine-tuning: the backbone and the BiFPN are frozen and run as the
inference plan's launches, every BN stays on its running statistics (the reference model's ``freeze_bn()``), and the
``regressor.*`` / ``classifier.*`` parameters get gradients.

``HeadTrain`` belongs to one inference plan (one batch size).  Its forward runs the heads with the inference kernels -- ``reg`` and
``cls`` equal the inference plan's bit for bit -- and keeps what the backward needs: every depthwise output, and the pre-activation
``z`` of every swish, written by the pointwise launch that applies it (stl_det_pointwise_train).  Its backward walks each (head,
level) from the header down through csrc/detector_train.hip and produces gradients of the *folded* weights W' = W s, b' = b s + t
(s, t the frozen BN's scale and shift) per level; ``fold_chain`` carries them to W, b, gamma and beta in a few elementwise torch
ops, and the weights shared by the five levels sum their five contributions.  The first depthwise layer of a (head, level) reads
a frozen feature map: no data gradient is computed for it.

``model.set_train_bifpn(k)`` (1 <= k <= cells - 1, or "all": below) trains the last k BiFPN cells with the heads, fp32 only.  The forward is not
touched: the inference plan keeps every map (``_Plan.cells``), and the backward recomputes each node's pre-activation from them.
Then the first depthwise layer of every (head, level) also computes its data gradient (stl_det_dwconv_bwd_data without z), the two
heads' gradients of a level are added regressor first, each times the gradient of its own loss (stl_det_grad_add reads the two
scalars on the device), and the cells run in reverse, the nodes of a cell in the reverse of the forward order.  Every consumer of a
map comes later in the forward order, so a map's gradient is complete when its node is reached; the first contribution writes, the
later ones accumulate, in that fixed order.  Per node: the pointwise layer's weight and data gradient (x = d), the depthwise
layer's weight gradient (x = f) and data gradient, then stl_det_fuse_bwd (csrc/detector_bifpn.hip), whose destinations are null for
the frozen inputs of the first trainable cell.  ``cell_raw_grads`` carries the folded gradients to the raw parameters: ``fold_chain``
for the pointwise layer and its BN, ``fusion_weight_grads`` for ``p*_w1`` / ``p*_w2``.

``model.set_train_bifpn("all")`` trains the first cell too, so everything behind the frozen backbone.  Its eight nodes run through the
same loop; their inputs are the seven maps the cell makes from P3 / P4 / P5 (``p3_in``, ``p4_in``, ``p5_in``, the second ``p4_in`` /
``p5_in`` of the down path, ``p6``, ``p7``), which get gradient maps like any node output.  Behind the nodes: stl_det_pool_bwd
(csrc/detector_bifpn.hip) of ``p6 -> p7``, adding to the gradient of ``p6``, then of ``t -> p6`` (``t`` the output of ``p5_to_p6``'s
conv and BN), then the weight gradients of the six 1x1 layers (stl_det_pointwise_bwd_weight with x = the backbone map: ``p5_to_p6``,
the three ``*_down_channel``, the two ``*_down_channel_2``; ``_Plan.first_pools`` / ``first_convs``).  No data gradient is computed for
P3 / P4 / P5: nothing before them trains.  ``fold_chain`` carries each folded pair to the conv's weight and bias and the BN's.

``model.set_train_backbone(k)`` (needs "all"; fp32) trains the last k MBConv blocks of the backbone's final stage too (block 15 of D0,
blocks 24 / 25 of D3: 3x3 stride-1 depthwise layers).  The forward is the inference forward (no drop-connect, BN on running
statistics); ``_Plan.blocks`` keeps each block's input, expand output e, depthwise output a, gate g and output.  Behind the cells'
launches (``_blocks_bwd``): stl_det_pointwise_bwd_data of ``p5_to_p6``, ``p5_down_channel`` and ``p5_down_channel_2`` into a buffer
each, joined in that order by stl_det_grad_add -- the gradient of P5; then per block, the last first, with the folded weights: D = dy
Wp'^T (stl_det_pointwise_bwd_data); stl_det_mbconv_gate_bwd (csrc/detector_mbconv.hip: xs = a g, sum a, sum D a); the projection's
weight gradient with x = xs; stl_det_se_bwd (dpool and the four SE gradients); the depthwise pre-activation u recomputed by
stl_det_dwconv at act 0; stl_det_mbconv_act_bwd (du = (D g + dpool / HW) swish'(u) over D, and the folded BN's bias gradient);
stl_det_dwconv_bwd_weight (x = e); the expand layer's pre-activation recomputed by stl_det_pointwise at act 0;
stl_det_dwconv_bwd_data (times swish' of it); the expand layer's weight gradient (x = the block input); and, where the block in front
trains too, its data gradient plus dy through the skip.  ``block_raw_grads`` carries the folded gradients to the raw parameters
(``fold_chain`` without a conv bias, ``dw_fold_chain``).  P3 / P4 and every block in front stay frozen.

``model.set_train_trunk(k)`` reaches further back: the last k blocks of the whole backbone, ``"all"`` the stem too.  The final stage's
blocks keep the launches above; a block in front of it runs the same sequence with stl_det_dwconv_bwd_weight_ks / _data_ks
(csrc/detector_trunk.hip: k 3 / 5, s 1 / 2 under TF "same" padding), the projection, gate, SE and act steps at the block's output
resolution, the expand recompute, the depthwise data gradient and the expand gradients at its input resolution.  A block without an
expand layer (e = 1) has no ``exp_w`` / ``exp_b``: its depthwise layer reads the block input, and stl_det_dwconv_bwd_data_ks without z
is the input's gradient.  The gradient of a block's input is joined in a fixed order: the block's own data gradient, dy through the
skip, then -- where the input is P4 / P3, the inputs of the last two stride-2 blocks -- stl_det_pointwise_bwd_data of
``p4_down_channel`` and ``p4_down_channel_2`` / of ``p3_down_channel``, each into a buffer of its own and added by stl_det_grad_add.
``tr.block_dy[i]`` keeps the joined gradient of block i's output, ``tr.stem_dy`` that of the stem's.  With the stem, block 0 also
produces its input's gradient and stl_det_stem_bwd follows (the pre-activation recomputed from the canvas the forward read; no image
gradient); its ``[3][3][3][Co]`` gradient is permuted to ``[Co, 3, 3, 3]`` and folded through ``_bn0`` as a conv without bias.

A model with ``compute_dtype="f16"`` trains in 16 bit, by the recipe of the pose network's mixed mode: the trunk runs as the 16-bit
inference plan's launches, the heads' forward tensors (every depthwise output d, pre-activation z and swish output t) are f16, the
gradients in flight are bf16, every sum is fp32, and the folded gradients come out in the same fp32 ``grads`` tensors, so
``fold_chain`` and ``raw_grads`` do not change (the contract is stated in include/stlpose_hip.h at stl_det_pointwise16_train).  The
data gradient of a pointwise layer reads a bf16 transposed pack of the folded weight (efficientdet.pack_transposed).  ``"bf16"`` does
not train: its forward error is several times that of f16.
"""
from __future__ import annotations

import ctypes
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


# ------------------------------------------------------------------------------------------------ launches
class HeadTrain:
    """Training forward and backward of the two heads on the features of one inference plan (efficientdet._Plan)."""

    def __init__(self, m, plan):
        self.B, self.dev = B, dev = plan.B, plan.dev
        self.generation = 0   # forwards through these buffers (the stale-backward check of _DetLossFn)
        self.fwd = LaunchList()
        self.bwd = LaunchList(self.fwd.keep)
        self.hdr = {h: [] for h in HEADS}   # the headers' backward descriptors, the very objects `bwd` passes by reference: set_grads sets their dy
        L = m._layout
        c, A, nc = m.fpn_channels, m.num_anchors_total, m.num_classes
        self.c, self.nlayers = c, len(m.regressor.conv_list)
        self.reg = torch.empty(B, A, 4, device=dev)
        self.cls = torch.empty(B, A, nc, device=dev)
        lib = capi.lib()
        h0 = plan.feats[0][1]
        m0 = B * h0 * h0
        self.h16, self.code, self.adtype = plan.h16, plan.code, plan.adtype   # 16-bit: d / z / t in adtype, ga / gb bf16
        if self.h16:
            m._ensure_transposed()
            self.wbufT, self.layoutT = m._wbufT16, m._layoutT
        gdtype = torch.bfloat16 if self.h16 else torch.float32
        self.ga, self.gb = torch.empty(m0 * c, device=dev, dtype=gdtype), torch.empty(m0 * c, device=dev, dtype=gdtype)   # gradients in flight, reused
        kmax = max(c, 9 * max(4, nc))
        slabs = getattr(lib, self._name("stl_det_pointwise_bwd_slabs"))
        self.ncells = ncells = m.train_bifpn   # the trailing BiFPN cells that train with the heads
        self.first = ncells == len(plan.cells)   # every cell: the first one's 1x1 layers (Ci = the backbone's channels) and plain pools too
        self.nblocks = nblocks = getattr(m, "train_backbone", 0)   # the trailing MBConv blocks that train with them
        self.stem = bool(getattr(m, "train_stem", False))          # and the stem (with every block)
        self.own_canvas = plan.canvas.data_ptr()
        assert not nblocks or self.first, "the backbone's blocks train with every BiFPN cell only"
        assert not self.stem or nblocks == len(plan.blocks), "the stem trains with every block only"
        npart = slabs(m0) * (c * kmax + kmax)
        if self.first:   # the largest slabs * (Ci * Co + Co) that is listed
            npart = max([npart] + [slabs(x.numel() // x.shape[3]) * (x.shape[3] * c + c) for x, _, _ in plan.first_convs.values()])
        for inp, e, a, _, y in plan.blocks[len(plan.blocks) - nblocks:]:   # the blocks' expand (input resolution) and project layers
            ci, mid, co = inp.shape[3], a.shape[3], y.shape[3]
            npart = max(npart, slabs(a.numel() // mid) * (mid * co + co))
            if e is not None:
                npart = max(npart, slabs(e.numel() // mid) * (ci * mid + mid))
        self.pw_part = torch.empty(npart, device=dev)
        self.dw_part = torch.empty(getattr(lib, self._name("stl_det_dwconv_bwd_parts"))(m0) * 9 * c, device=dev)
        self.grads: Dict[str, Dict[str, torch.Tensor]] = {}
        if ncells:
            assert not self.h16, "the BiFPN cells train in fp32 only"
            # the gradient of every node output of the trainable cells, by the address of the plan's map
            self.gmap = {y.data_ptr(): torch.empty_like(y) for kept in plan.cells[len(plan.cells) - ncells:] for _, _, y, _, _ in kept.values()}
            if self.first:   # and of the first cell's seven input maps (p3_in, p4_in, p5_in, p4_in_2, p5_in_2, p6, p7) and of t
                for y in [y for _, y, _ in plan.first_convs.values()] + [y for _, _, y in plan.first_pools]:
                    self.gmap[y.data_ptr()] = torch.empty_like(y)
            self.hc = [torch.empty_like(f) for f, _ in plan.feats]   # the classifier's gradient of each level (the regressor's goes to gmap)
            self.scale = torch.ones(2, device=dev)                   # the gradients of (regression, classification): _DetLossFn.backward
        for name, out, k, act in (("regressor", self.reg, 4, 0), ("classifier", self.cls, nc, 2)):
            lay, n = L[name], self.nlayers
            g = dict(pw_w=torch.empty(5, n, c, c, device=dev), pw_b=torch.empty(5, n, c, device=dev),
                     dw=torch.empty(5, n, 3, 3, c, device=dev), hpw_w=torch.empty(5, c, 9 * k, device=dev),
                     hpw_b=torch.empty(5, 9 * k, device=dev), hdw=torch.empty(5, 3, 3, c, device=dev))
            self.grads[name] = g
            aoff = 0
            for lv, (f, hh) in enumerate(plan.feats):
                M = B * hh * hh
                buf = lambda: torch.empty(B, hh, hh, c, device=dev, dtype=self.adtype)   # noqa: E731
                t, d, z = [f], [], []
                for i in range(n):
                    d.append(buf()), z.append(buf()), t.append(buf())
                    list_dwconv(self.fwd, self.code, t[i], plan._w(lay["dw"][i]), None, d[i], B, hh, c, 3, 1, 0)
                    list_pointwise(self.fwd, self.code, plan.pw_fields(d[i], t[i + 1], hh * hh, c, c, lay["pw"][lv][i], 1), False, z=z[i])
                dh = buf()
                list_dwconv(self.fwd, self.code, t[n], plan._w(lay["hdw"]), None, dh, B, hh, c, 3, 1, 0)
                strides = dict(img_stride=A * k, row_stride=9 * k, off=aoff * k)
                list_pointwise(self.fwd, self.code, plan.pw_fields(dh, out, hh * hh, c, 9 * k, lay["hpw"], act, **strides), True)
                self.fwd.keep_alive(*d, *t, dh)   # the pointwise descriptors hold their addresses
                # backward, from the header down; ga / gb alternate as the gradient of a depthwise / a pointwise output
                self.hdr[name].append(self._pw_bwd(plan, dh, None, self.ga, M, hh * hh, c, 9 * k, lay["hpw"], g["hpw_w"][lv],
                                                   g["hpw_b"][lv], **strides))
                self._dw_bwd(t[n], self.ga, plan._w(lay["hdw"]), g["hdw"][lv], z[n - 1], self.gb, hh)
                for i in range(n - 1, -1, -1):
                    self._pw_bwd(plan, d[i], self.gb, self.ga, M, hh * hh, c, c, lay["pw"][lv][i], g["pw_w"][lv, i], g["pw_b"][lv, i])
                    dx0 = None if not ncells else (self.gmap[f.data_ptr()] if name == "regressor" else self.hc[lv])
                    self._dw_bwd(t[i], self.ga, plan._w(lay["dw"][i]), g["dw"][lv, i], z[i - 1] if i else None, self.gb if i else dx0, hh)
                aoff += hh * hh * 9
        if ncells:
            self._cells_bwd(plan, L)
        self.bgrads = {}
        if nblocks:
            self._blocks_bwd(m, plan, L)

    def _cells_bwd(self, plan, L) -> None:
        """The backward launches of the trainable cells, behind the heads'."""
        B, c, dev = self.B, self.c, self.dev
        written = set()   # the maps whose gradient has its first contribution
        for lv, (f, _) in enumerate(plan.feats):
            g = self.gmap[f.data_ptr()]
            self.bwd.add("stl_det_grad_add", g, self.hc[lv], self.scale, self.scale[1:], g, g.numel())
            written.add(f.data_ptr())
        self.fuse_ws = torch.empty(capi.lib().stl_det_fuse_bwd_workspace(self.ga.numel()), device=dev)
        first = len(plan.cells) - self.ncells
        self.cgrads = {}
        for j in range(len(plan.cells) - 1, first - 1, -1):
            lay, kept = L["bifpn"][j], plan.cells[j]
            for name in reversed(_BiFPN.NODES):   # the forward runs them in this tuple's order
                f, d, y, desc, terms = kept[name]
                assert y.data_ptr() in written, (j, name)
                h = y.shape[1]
                g = dict(pw_w=torch.empty(c, c, device=dev), pw_b=torch.empty(c, device=dev), dw=torch.empty(3, 3, c, device=dev),
                         what=torch.zeros(3, device=dev))
                self.cgrads[j, name] = g
                self._pw_bwd(plan, d, self.gmap[y.data_ptr()], self.ga, B * h * h, h * h, c, c, lay[name][1], g["pw_w"], g["pw_b"])
                self._dw_bwd(f, self.ga, plan._w(lay[name][0]), g["dw"], None, self.gb, h)
                fb = capi.DetFuseBwd()
                for i, t in enumerate(terms):   # a term outside gmap is an input of the first trainable cell: frozen
                    dst = self.gmap.get(t.data_ptr())
                    if dst is not None:
                        fb.dx[i], fb.accumulate[i] = dst.data_ptr(), int(t.data_ptr() in written)
                        written.add(t.data_ptr())
                self.bwd.keep_alive(f, d, y, *terms)   # the descriptors hold their addresses
                self.bwd.add("stl_det_fuse_bwd", desc, self.gb, fb, self.fuse_ws, g["what"])
        self.fgrads = {}
        if not self.first:
            return
        # behind the first cell's nodes: p6 -> p7 adds to g(p6), which is complete then; t -> p6 writes g(t); then the weight gradients
        # of the six 1x1 layers, x the frozen backbone map (no data gradient: nothing trains before them), p5_to_p6 first
        for desc, x, y in reversed(plan.first_pools):
            assert y.data_ptr() in written, "a pooled map of the first cell without a gradient"
            self.bwd.keep_alive(x, y)
            self.bwd.add("stl_det_pool_bwd", desc, self.gmap[y.data_ptr()], self.gmap[x.data_ptr()], int(x.data_ptr() in written))
            written.add(x.data_ptr())
        order = ("p5_to_p6", "p3_down_channel", "p4_down_channel", "p5_down_channel", "p4_down_channel_2", "p5_down_channel_2")
        assert sorted(order) == sorted(plan.first_convs)
        for key in order:
            x, y, pk = plan.first_convs[key]
            assert y.data_ptr() in written, key
            ci, hw = x.shape[3], x.shape[1] * x.shape[2]
            g = self.fgrads[key] = dict(pw_w=torch.empty(ci, c, device=dev), pw_b=torch.empty(c, device=dev))
            dy = self.gmap[y.data_ptr()]
            p = capi.DetPointwiseBwd(x.data_ptr(), None, dy.data_ptr(), None, g["pw_w"].data_ptr(), g["pw_b"].data_ptr(),
                                     self.pw_part.data_ptr(), B * hw, hw * c, c, 0, hw, ci, c, pk[2], pk[3], 0)
            self.bwd.keep_alive(x, dy, g["pw_w"], g["pw_b"])   # the descriptor holds their addresses
            self.bwd.add("stl_det_pointwise_bwd_weight", p)

    def _pw_bwd_data(self, plan, pk, dy, dx, hw, ci, co) -> None:
        """The data gradient alone of the pointwise layer packed as pk: dx [B hw, ci] = dy [B hw, co] W'^T."""
        p = capi.DetPointwiseBwd(None, plan.wbuf[pk[0]:].data_ptr(), dy.data_ptr(), dx.data_ptr(), None, None, None, self.B * hw, hw * co,
                                 co, 0, hw, ci, co, pk[2], pk[3], 0)
        self.bwd.keep_alive(dy, dx)   # the descriptor holds their addresses
        self.bwd.add("stl_det_pointwise_bwd_data", p)

    def _pw_bwd_weight(self, pk, x, dy, gw, gb, hw, ci, co) -> None:
        """The weight and bias gradient alone of the pointwise layer packed as pk, x [B hw, ci], dy [B hw, co]."""
        p = capi.DetPointwiseBwd(x.data_ptr(), None, dy.data_ptr(), None, gw.data_ptr(), gb.data_ptr(), self.pw_part.data_ptr(),
                                 self.B * hw, hw * co, co, 0, hw, ci, co, pk[2], pk[3], 0)
        self.bwd.keep_alive(x, dy, gw, gb)   # the descriptor holds their addresses
        self.bwd.add("stl_det_pointwise_bwd_weight", p)

    def _join(self, plan, dx, x, keys) -> None:
        """dx, the gradient of the backbone map x, += the data gradients of the first cell's 1x1 layers `keys` that read x: each into a
        buffer of its own, added in the order of `keys`."""
        hw, ci = x.shape[1] * x.shape[2], x.shape[3]
        for key in keys:
            xx, y, pk = plan.first_convs[key]
            assert xx is x, key
            t = torch.empty_like(x)
            self._pw_bwd_data(plan, pk, self.gmap[y.data_ptr()], t, hw, ci, self.c)
            self.bwd.add("stl_det_grad_add", dx, t, None, None, dx, dx.numel())
            self.bwd.keep_alive(t)

    def _blocks_bwd(self, m, plan, L) -> None:
        """The backward launches of the trainable MBConv blocks (csrc/detector_mbconv.hip, csrc/detector_trunk.hip), behind the cells':
        the data gradient of P5 through the three 1x1 layers of the first cell that read it, then the blocks, the last one first, then
        the stem's weight gradient when it trains."""
        B, dev, lib = self.B, self.dev, capi.lib()
        net = m.backbone_net.model
        specs, nb = net.specs, len(plan.blocks)
        p3, p4, p5 = plan.backbone
        h, c5 = p5.shape[1], p5.shape[3]
        assert plan.blocks[-1][4] is p5
        self.blocks_start = len(self.bwd)   # bwd.calls[blocks_start:] are these launches
        parts = []
        for key in ("p5_to_p6", "p5_down_channel", "p5_down_channel_2"):   # each into a buffer of its own, joined in this order
            x, y, pk = plan.first_convs[key]
            assert x is p5, key
            parts.append(torch.empty_like(p5))
            self._pw_bwd_data(plan, pk, self.gmap[y.data_ptr()], parts[-1], h * h, c5, self.c)
        dy = self.gp5 = parts[0]   # the gradient of P5
        for t in parts[1:]:
            self.bwd.add("stl_det_grad_add", dy, t, None, None, dy, dy.numel())
        self.bwd.keep_alive(*parts)
        first = nb - self.nblocks
        heads_form = nb - m.final_stage_blocks()   # from this block on: 3 x 3 / 1, the heads' depthwise backward entry points
        todo = range(first, nb)
        mids = [specs[i]["mid"] for i in todo]
        ses = [specs[i]["se"] for i in todo]
        hin = [plan.blocks[i][0].shape[1] for i in todo]
        hout = [plan.blocks[i][2].shape[1] for i in todo]
        # scratch shared by the blocks, sized for the largest h^2 mid among them: D / du (output resolution); xs / u (output) and z_e
        # (input resolution); dz_e (input resolution); and the small ones
        n1 = max(ho * ho * mid for ho, mid in zip(hout, mids))
        n2 = max(max(ho * ho, hi * hi if specs[i]["e"] != 1 else 0) * mid for i, hi, ho, mid in zip(todo, hin, hout, mids))
        n3 = max([hi * hi * mid for i, hi, mid in zip(todo, hin, mids) if specs[i]["e"] != 1] + [1])
        s1, s2, s3 = (torch.empty(B * n, device=dev) for n in (n1, n2, n3))
        gate_ws = torch.empty(max(lib.stl_det_mbconv_gate_bwd_workspace(B, ho * ho, mid) for ho, mid in zip(hout, mids)), device=dev)
        act_ws = torch.empty(max(lib.stl_det_mbconv_act_bwd_workspace(B, ho * ho, mid) for ho, mid in zip(hout, mids)), device=dev)
        se_ws = torch.empty(max(lib.stl_det_se_bwd_workspace(B, mid, cs) for mid, cs in zip(mids, ses)), device=dev)
        asum, dgate, dpool = (torch.empty(B * max(mids), device=dev) for _ in range(3))
        dwb_part = torch.empty(lib.stl_det_dwconv_bwd_parts(B * h * h) * 9 * max(mids[max(heads_form - first, 0):]), device=dev)
        ks_part = torch.empty(max([lib.stl_det_dwconv_bwd_ks_parts(B * ho * ho) * specs[i]["k"] ** 2 * mid
                                   for i, ho, mid in zip(todo, hout, mids) if i < heads_form] + [1]), device=dev)
        self.bwd.keep_alive(s1, s2, s3, gate_ws, act_ws, se_ws, asum, dgate, dpool, dwb_part, ks_part)
        self.block_dy = {}   # block -> the gradient of its output, after every join
        self.stem_dy = None  # the gradient of the stem's output (train_stem)
        for i in range(nb - 1, first - 1, -1):
            b, lay = specs[i], L["blocks"][i]
            inp, e, a, gate, y = plan.blocks[i]
            ci, mid, co, cs, k, s = b["ci"], b["mid"], b["co"], b["se"], b["k"], b["s"]
            hi, ho = inp.shape[1], a.shape[1]
            hwi, hwo = hi * hi, ho * ho
            old = i >= heads_form
            assert dy.shape == y.shape and (e is None) == (b["e"] == 1) and ho == (hi + s - 1) // s, i
            assert not old or (k == 3 and s == 1 and e is not None), i
            self.block_dy[i] = dy
            g = self.bgrads[i] = dict(exp_w=torch.empty(ci, mid, device=dev), exp_b=torch.empty(mid, device=dev)) if e is not None else {}
            g.update(dw=torch.empty(k, k, mid, device=dev), dw_b=torch.empty(mid, device=dev),
                     se_w1=torch.empty(cs, mid, device=dev), se_b1=torch.empty(cs, device=dev),
                     se_w2=torch.empty(mid, cs, device=dev), se_b2=torch.empty(mid, device=dev),
                     proj_w=torch.empty(mid, co, device=dev), proj_b=torch.empty(co, device=dev))
            self.bwd.keep_alive(inp, e, a, gate, y, *g.values())
            wd, bd = plan._w(lay["dw"][0]), plan._w(lay["dw"][1])
            xd = inp if e is None else e   # what the depthwise layer reads
            # the projection: D = dy Wp'^T; xs = a g, asum, dgate; dWp', dbp' with x = xs
            self._pw_bwd_data(plan, lay["project"], dy, s1, hwo, mid, co)
            self.bwd.add("stl_det_mbconv_gate_bwd", a, s1, gate, s2, gate_ws, asum, dgate, B, hwo, mid)
            self._pw_bwd_weight(lay["project"], s2, dy, g["proj_w"], g["proj_b"], hwo, mid, co)
            # the gate: dpool and the SE gradients
            self.bwd.add("stl_det_se_bwd", asum, dgate, gate, B, hwo, mid, cs, *[plan._w(o) for o in lay["se"]], se_ws, dpool,
                         g["se_w1"], g["se_b1"], g["se_w2"], g["se_b2"])
            # the depthwise layer: u recomputed by the forward's launch without the activation; du overwrites D; db_d'; dw_d'
            list_dwconv(self.bwd, 0, xd, wd, bd, s2, B, hi, mid, k, s, 0)
            self.bwd.add("stl_det_mbconv_act_bwd", s1, s2, gate, dpool, s1, act_ws, g["dw_b"], B, hwo, mid)
            if old:
                self.bwd.add("stl_det_dwconv_bwd_weight", xd, s1, dwb_part, g["dw"], B, hi, hi, mid)
            else:
                self.bwd.add("stl_det_dwconv_bwd_weight_ks", xd, s1, ks_part, g["dw"], B, hi, hi, mid, k, s)
            need_dx = i > first or self.stem   # the block (or the stem) in front trains too: the gradient of this block's input
            dx = torch.empty_like(inp) if need_dx else None
            if e is not None:
                # the expand layer: its pre-activation z_e recomputed the same way, dz_e = dwconv^T(du) swish'(z_e); dWe', dbe'
                list_pointwise(self.bwd, 0, plan.pw_fields(inp, s2, hwi, ci, mid, lay["expand"], 0), False)
                if old:
                    self.bwd.add("stl_det_dwconv_bwd_data", s1, wd, s2, s3, B, hi, hi, mid)
                else:
                    self.bwd.add("stl_det_dwconv_bwd_data_ks", s1, wd, s2, s3, B, hi, hi, mid, k, s)
                self._pw_bwd_weight(lay["expand"], inp, s3, g["exp_w"], g["exp_b"], hwi, ci, mid)
                if need_dx:
                    self._pw_bwd_data(plan, lay["expand"], s3, dx, hwi, ci, mid)
            elif need_dx:   # no expand layer: the depthwise layer reads the block input, its data gradient is the input's
                self.bwd.add("stl_det_dwconv_bwd_data_ks", s1, wd, None, dx, B, hi, hi, mid, k, s)
            if need_dx:
                # joined in this order: the block's own data gradient, dy through the skip, then -- where the input is P4 / P3 -- the
                # data gradients of the first cell's 1x1 layers that read it: p4_down_channel, p4_down_channel_2 / p3_down_channel
                if b["skip"]:
                    self.bwd.add("stl_det_grad_add", dx, dy, None, None, dx, dx.numel())
                if inp is p4:
                    self._join(plan, dx, p4, ("p4_down_channel", "p4_down_channel_2"))
                elif inp is p3:
                    self._join(plan, dx, p3, ("p3_down_channel",))
                dy = dx
        if self.stem:
            assert first == 0 and dy.shape == plan.blocks[0][0].shape
            self.stem_dy = dy
            S, co = plan.canvas.shape[1], dy.shape[3]
            ho = dy.shape[1]
            self.sgrads = dict(w=torch.empty(3, 3, 3, co, device=dev), b=torch.empty(co, device=dev))
            stem_part = torch.empty(lib.stl_det_stem_bwd_parts(B * ho * ho) * 28 * co, device=dev)
            # the canvas the forward read: the plan's own, or the batch's (set_canvas before each backward)
            self.canvas_arg = ctypes.c_void_p(plan.canvas.data_ptr())
            self.bwd.keep_alive(plan.canvas, dy, stem_part, *self.sgrads.values())
            self.bwd.add("stl_det_stem_bwd", self.canvas_arg, plan._w(L["stem"][0]), plan._w(L["stem"][1]), dy, stem_part, self.sgrads["w"],
                         self.sgrads["b"], B, S, S, co)

    def set_canvas(self, canvas) -> None:
        """The canvas the forward about to be differentiated read (None: the plan's own); the caller keeps it alive until the backward."""
        if self.stem:
            self.canvas_arg.value = self.own_canvas if canvas is None else canvas.data_ptr()

    def _name(self, name: str) -> str:
        return NAME16[name] if self.h16 else name

    def _pw_bwd(self, plan, x, dy, dx, M, hw, ci, co, pk, gw, gb, img_stride=None, row_stride=None, off=0):
        """Weight and data gradient of one pointwise layer; dy None: a header, whose dy (dreg / dlogit, fp32) set_grads fills in."""
        w, _, kp, np_ = pk
        ptrs = (None if dy is None else dy.data_ptr(), dx.data_ptr(), gw.data_ptr(), gb.data_ptr(), self.pw_part.data_ptr(), M,
                hw * co if img_stride is None else img_stride, co if row_stride is None else row_stride, off, hw, ci, co)
        if self.h16:
            wt, kt, nt = self.layoutT[w]
            p = capi.DetPointwise16Bwd(x.data_ptr(), self.wbufT[wt:].data_ptr(), *ptrs, kt, nt, self.code, 1 if dy is None else 0, 0)
        else:
            p = capi.DetPointwiseBwd(x.data_ptr(), plan.wbuf[w:].data_ptr(), *ptrs, kp, np_, 0)
        self.bwd.keep_alive(x, gw, gb)   # the descriptor holds their addresses
        self.bwd.add(self._name("stl_det_pointwise_bwd_weight"), p)
        self.bwd.add(self._name("stl_det_pointwise_bwd_data"), p)
        return p

    def _dw_bwd(self, x, dy, w, gw, z, dx, h):
        """Weight gradient of one depthwise layer and, with dx, its data gradient times swish'(z) of the layer below."""
        code = (self.code,) if self.h16 else ()   # the 16-bit entry points take the forward tensors' type: first / last argument
        self.bwd.add(self._name("stl_det_dwconv_bwd_weight"), *code, x, dy, self.dw_part, gw, self.B, h, h, self.c)
        if dx is not None:
            self.bwd.add(self._name("stl_det_dwconv_bwd_data"), dy, w, z, dx, self.B, h, h, self.c, *code)

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
    kb = getattr(m, "train_backbone", 0)
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
        pw, bn = sep.pointwise_conv.conv, sep.bn
        W, b = pw.weight.detach().reshape(pw.out_channels, pw.in_channels), pw.bias.detach()
        dW, db, dgam, dbeta = fold_chain(W, b, bn.weight.detach(), bn.running_mean, bn.running_var, bn.eps, g["pw_w"].t(), g["pw_b"])
        out[pre + "pointwise_conv.conv.weight"], out[pre + "pointwise_conv.conv.bias"] = dW[:, :, None, None], db
        out[pre + "bn.weight"], out[pre + "bn.bias"] = dgam, dbeta.clone()
        wname = dict(zip(_BiFPN.NODES, _BiFPN.WEIGHTS))[node][0]
        p = getattr(m.bifpn[j], wname).detach()
        out[f"bifpn.{j}.{wname}"] = fusion_weight_grads(p, g["what"][:p.numel()])
    for key, g in tr.fgrads.items():   # the first cell's 1x1 layers: Sequential(conv, BN[, pool])
        seq, pre = getattr(m.bifpn[0], key), f"bifpn.0.{key}."
        pw, bn = seq[0].conv, seq[1]
        W, b = pw.weight.detach().reshape(pw.out_channels, pw.in_channels), pw.bias.detach()
        dW, db, dgam, dbeta = fold_chain(W, b, bn.weight.detach(), bn.running_mean, bn.running_var, bn.eps, g["pw_w"].t(), g["pw_b"])
        out[pre + "0.conv.weight"], out[pre + "0.conv.bias"] = dW[:, :, None, None], db
        out[pre + "1.weight"], out[pre + "1.bias"] = dgam, dbeta.clone()
    return out


def block_raw_grads(m, tr: HeadTrain) -> Dict[str, torch.Tensor]:
    """{parameter name: gradient} of every parameter of the trainable MBConv blocks from the folded per-block gradients of tr: the
    two pointwise layers by ``fold_chain`` (convs without bias), the depthwise layer by ``dw_fold_chain``, the SE convs as they are."""
    out = {}
    for i, g in tr.bgrads.items():
        blk, pre = m.backbone_net.model._blocks[i], f"backbone_net.model._blocks.{i}."
        layers = [("_expand_conv", "_bn0", g["exp_w"], g["exp_b"])] if "exp_w" in g else []   # (a block without an expand layer)
        for conv, bn, gw, gb in layers + [("_project_conv", "_bn2", g["proj_w"], g["proj_b"])]:
            pw, n = getattr(blk, conv).conv, getattr(blk, bn)
            W = pw.weight.detach().reshape(pw.out_channels, pw.in_channels)
            dW, _, dgam, dbeta = fold_chain(W, None, n.weight.detach(), n.running_mean, n.running_var, n.eps, gw.t(), gb)
            out[pre + conv + ".conv.weight"] = dW[:, :, None, None]
            out[pre + bn + ".weight"], out[pre + bn + ".bias"] = dgam, dbeta.clone()
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
            pre = f"{h}.conv_list.{i}."
            out[pre + "depthwise_conv.conv.weight"] = g["dw"][:, i].sum(0).permute(2, 0, 1)[:, None]
            pw = cv.pointwise_conv.conv
            W, b = pw.weight.detach().reshape(pw.out_channels, pw.in_channels), pw.bias.detach()
            dW, db = torch.zeros_like(W), torch.zeros_like(b)
            for lv in range(5):
                bn = hd.bn_list[lv][i]
                a, bb, dgam, dbeta = fold_chain(W, b, bn.weight.detach(), bn.running_mean, bn.running_var, bn.eps,
                                                g["pw_w"][lv, i].t(), g["pw_b"][lv, i])
                dW, db = dW + a, db + bb
                out[f"{h}.bn_list.{lv}.{i}.weight"], out[f"{h}.bn_list.{lv}.{i}.bias"] = dgam, dbeta.clone()
            out[pre + "pointwise_conv.conv.weight"], out[pre + "pointwise_conv.conv.bias"] = dW[:, :, None, None], db
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
