"""EfficientDet person detector on MI355X (mirror of reference ``src/models/EfficientDet.py`` with
``models/efficientdet_utils/{model,utils}.py`` and ``models/efficientnet/{model,utils,utils_extra}.py``).

``EfficientDetBackbone(num_classes, compound_coef)`` holds the reference's parameters and buffers under the reference's key names
(a reference checkpoint loads with ``strict=True``, also with the ``module.`` prefix of a DataParallel save).  Its forward is
inference only (``detection_loss`` fine-tunes the heads, see below) and runs every layer through csrc/detector.hip (NHWC): the preprocess kernel, the stem, depthwise and
squeeze-excitation kernels, the pointwise GEMM on MFMA with BN folded into its weights, the BiFPN node kernel, the shared
heads writing straight into the concatenated outputs, the decode kernel and the class-aware NMS.  BN is folded into packed fp32
weights on the device and refolded when any parameter or buffer changes (only the tail of the buffer, in place, when only the
trainable BiFPN cells or ``regressor.*`` / ``classifier.*`` changed: an optimiser step of the fine-tuning keeps the plans); the launches of one batch size
are listed once (``_Plan``) and replayed; the last MAX_PLANS batch sizes keep their plans.  Only the kept boxes, scores and labels reach the host.

``compute_dtype`` is "fp32" (the default), "bf16" or "f16".  Parameters, buffers and ``state_dict()`` are fp32 in every mode and
BN is folded in fp64; a 16-bit mode stores the activations between the stem and the head outputs in that type (the canvas, the
head outputs ``reg`` / ``cls``, decode and NMS stay fp32), rounds the folded pointwise weights once to it for the 16-bit MFMA and
keeps every other weight, every bias and every sum in fp32.  The depthwise kernel of an MBConv block also writes the
squeeze-excitation pooling sums, so a 16-bit plan has no pooling pass.  In "f16" a forward whose head outputs hold a non-finite
value raises FloatingPointError (activations left f16's range: use "bf16"), as HRNet's "mixed" mode does.

``detection_loss(inputs, targets)`` ("fp32", or "f16" with bf16 gradients in flight and fp32 ``.grad``; "bf16" raises;
stlpose_amd/detector_train.py, csrc/detector_train.hip) is the first stage of
EfficientDet fine-tuning, the counterpart of ``loss_dict = model(imgs / 255, targets)`` in ``02_train_faster_rcnn.py:212``: the
backbone and the BiFPN are frozen, every BN stays on its running statistics, and ``sum(loss_dict.values()).backward()`` fills
``.grad`` of the ``regressor.*`` and ``classifier.*`` parameters.  ``set_train_bifpn(k)`` (fp32) is the next stage: the last k BiFPN
cells, 1 <= k <= cells - 1, train with the heads (csrc/detector_bifpn.hip; ``detector_train.trainable_parameters``); the cells before
them and the backbone stay frozen.  ``set_train_bifpn("all")`` trains every cell, the first one with its down-channel convs,
``p5_to_p6`` and the two plain pooled maps included: everything behind the backbone, which stays frozen unless
``set_train_backbone(k)`` (after "all"; fp32) also trains the last k MBConv blocks, 0 <= k <= the blocks of the final stage (1 for D0, 2
for D3: the ones that produce P5; csrc/detector_mbconv.hip).  The blocks are packed in front of the cells, so an optimiser step still
rewrites one tail of the weight buffer.  ``set_train_trunk(k)`` has no such limit: the last k blocks of the whole backbone, 0 <= k <= 16 /
26, and with ``"all"`` the stem too (``train_stem``; csrc/detector_trunk.hip: the depthwise backward at k 3 / 5, s 1 / 2 and the stem's
weight gradient), which is every parameter of the detector; the stem is packed first, so its step rewrites the whole buffer in place.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)
from .launch import LaunchList

BN_EPS = 1e-3
MAX_SIZE = 512   # preprocess canvas; the reference passes 512 for every compound_coef (EfficientDet.py:96)
MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
RATIOS = [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)]
SCALES = [2 ** 0, 2 ** (1.0 / 3.0), 2 ** (2.0 / 3.0)]
STRIDES = [8, 16, 32, 64, 128]

# EfficientDet.py:20-40, for the compound coefficients setup_detector allows
FPN_FILTERS = {0: 64, 3: 160}
FPN_REPEATS = {0: 3, 3: 6}
HEAD_REPEATS = {0: 3, 3: 4}
P345_CHANNELS = {0: (40, 112, 320), 3: (48, 136, 384)}
ANCHOR_SCALE = {0: 4.0, 3: 4.0}
# EfficientNet-B0 stages (efficientnet/utils.py:235-240): kernel, repeats, in, out, expand, stride; SE ratio 0.25 everywhere
STAGES = [(3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2), (5, 3, 80, 112, 6, 1),
          (5, 4, 112, 192, 6, 2), (3, 1, 192, 320, 6, 1)]
WIDTH_DEPTH = {0: (1.0, 1.0), 3: (1.2, 1.4)}   # efficientnet-b0 / -b3
# compute_dtype -> (activation dtype, the library's dtype code STL_F32 / STL_BF16 / STL_F16)
COMPUTE_DTYPES = {name: (capi.DTYPES[code][1], code) for name, code in (("fp32", capi.F32), ("bf16", capi.BF16), ("f16", capi.F16))}


def round_filters(f: int, width: float) -> int:
    x = f * width
    new = max(8, int(x + 4) // 8 * 8)
    return int(new + 8 if new < 0.9 * x else new)


def block_specs(cc: int) -> List[dict]:
    """The MBConv blocks of EfficientNet-b{cc}: in / out channels, kernel, stride, expansion, squeezed channels, identity skip.
    Like the reference, the skip is taken by the repeated blocks of a stage only (their stride is the integer 1)."""
    w, d = WIDTH_DEPTH[cc]
    out = []
    for k, r, i, o, e, s in STAGES:
        ci, co, rep = round_filters(i, w), round_filters(o, w), int(math.ceil(d * r))
        for j in range(rep):
            cin = ci if j == 0 else co
            out.append(dict(ci=cin, co=co, k=k, s=s if j == 0 else 1, e=e, mid=cin * e, se=max(1, int(cin * 0.25)), skip=j > 0 and cin == co))
    return out


# ------------------------------------------------------------------------------------------------ modules with the reference's keys
def _bn(c):
    return nn.BatchNorm2d(c, momentum=0.01, eps=BN_EPS)


class _SameConv(nn.Module):
    """Conv2dStaticSamePadding: the conv sits under ``.conv``."""

    def __init__(self, ci, co, k, stride=1, bias=True, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(ci, co, k, stride=stride, bias=bias, groups=groups)


class _Pool(nn.Module):
    """MaxPool2dStaticSamePadding(3, 2): no parameters."""


class _MBConv(nn.Module):
    def __init__(self, b):
        super().__init__()
        if b["e"] != 1:
            self._expand_conv = _SameConv(b["ci"], b["mid"], 1, bias=False)
            self._bn0 = _bn(b["mid"])
        self._depthwise_conv = _SameConv(b["mid"], b["mid"], b["k"], stride=b["s"], bias=False, groups=b["mid"])
        self._bn1 = _bn(b["mid"])
        self._se_reduce = _SameConv(b["mid"], b["se"], 1)
        self._se_expand = _SameConv(b["se"], b["mid"], 1)
        self._project_conv = _SameConv(b["mid"], b["co"], 1, bias=False)
        self._bn2 = _bn(b["co"])


class _EffNet(nn.Module):
    def __init__(self, cc):
        super().__init__()
        self.specs = block_specs(cc)
        c0 = round_filters(32, WIDTH_DEPTH[cc][0])
        self._conv_stem = _SameConv(3, c0, 3, stride=2, bias=False)
        self._bn0 = _bn(c0)
        self._blocks = nn.ModuleList([_MBConv(b) for b in self.specs])


class _Backbone(nn.Module):
    def __init__(self, cc):
        super().__init__()
        self.model = _EffNet(cc)


class _SepConv(nn.Module):
    def __init__(self, ci, co=None, norm=True):
        super().__init__()
        co = ci if co is None else co
        self.depthwise_conv = _SameConv(ci, ci, 3, bias=False, groups=ci)
        self.pointwise_conv = _SameConv(ci, co, 1)
        self.norm = norm
        if norm:
            self.bn = _bn(co)


class _BiFPN(nn.Module):
    NODES = ("conv6_up", "conv5_up", "conv4_up", "conv3_up", "conv4_down", "conv5_down", "conv6_down", "conv7_down")
    WEIGHTS = (("p6_w1", 2), ("p5_w1", 2), ("p4_w1", 2), ("p3_w1", 2), ("p4_w2", 3), ("p5_w2", 3), ("p6_w2", 3), ("p7_w2", 2))

    def __init__(self, c, p345, first):
        super().__init__()
        for n in self.NODES:
            setattr(self, n, _SepConv(c))
        self.first_time = first
        if first:
            self.p5_down_channel = nn.Sequential(_SameConv(p345[2], c, 1), _bn(c))
            self.p4_down_channel = nn.Sequential(_SameConv(p345[1], c, 1), _bn(c))
            self.p3_down_channel = nn.Sequential(_SameConv(p345[0], c, 1), _bn(c))
            self.p5_to_p6 = nn.Sequential(_SameConv(p345[2], c, 1), _bn(c), _Pool())
            self.p6_to_p7 = nn.Sequential(_Pool())
            self.p4_down_channel_2 = nn.Sequential(_SameConv(p345[1], c, 1), _bn(c))
            self.p5_down_channel_2 = nn.Sequential(_SameConv(p345[2], c, 1), _bn(c))
        for n, k in self.WEIGHTS:
            setattr(self, n, nn.Parameter(torch.ones(k, dtype=torch.float32)))


class _Head(nn.Module):
    def __init__(self, c, co, layers):
        super().__init__()
        self.conv_list = nn.ModuleList([_SepConv(c, c, norm=False) for _ in range(layers)])
        self.bn_list = nn.ModuleList([nn.ModuleList([_bn(c) for _ in range(layers)]) for _ in range(5)])
        self.header = _SepConv(c, co, norm=False)


# ------------------------------------------------------------------------------------------------ host-side reference pieces
def anchors(cc: int, image_hw=(MAX_SIZE, MAX_SIZE)) -> np.ndarray:
    """Anchors.forward (efficientdet_utils/utils.py:85-144): [A, 4] (y1, x1, y2, x2), built in float64, cast to float32."""
    h, w = image_hw
    out = []
    for stride in STRIDES:
        if w % stride:
            raise ValueError("input size must be divided by the stride.")
        level = []
        for scale in SCALES:
            for r in RATIOS:
                base = ANCHOR_SCALE[cc] * stride * scale
                ax, ay = base * r[0] / 2.0, base * r[1] / 2.0
                xv, yv = np.meshgrid(np.arange(stride / 2, w, stride), np.arange(stride / 2, h, stride))
                xv, yv = xv.reshape(-1), yv.reshape(-1)
                level.append(np.stack([yv - ay, xv - ax, yv + ay, xv + ax], 1)[:, None])
        out.append(np.concatenate(level, 1).reshape(-1, 4))
    return np.vstack(out).astype(np.float32)


def resize_meta(old_h: int, old_w: int, size: int = MAX_SIZE):
    """aspectaware_resize_padding's sizes (efficientdet_utils/utils.py:209-239), in Python float64: (new_w, new_h, old_w, old_h,
    padding_w, padding_h)."""
    if old_w > old_h:
        new_w, new_h = size, int(size / old_w * old_h)
    else:
        new_w, new_h = int(size / old_h * old_w), size
    return new_w, new_h, old_w, old_h, size - new_w, size - new_h


def invert_affine(meta, rois: np.ndarray) -> np.ndarray:
    """invert_affine (efficientdet_utils/utils.py:242-256): float32 rois divided by the float64 ratios, as numpy does it."""
    new_w, new_h, old_w, old_h = meta[:4]
    r = rois.copy()
    r[:, [0, 2]] = r[:, [0, 2]] / (new_w / old_w)
    r[:, [1, 3]] = r[:, [1, 3]] / (new_h / old_h)
    return r


def _device(dev) -> torch.device:
    """torch.device("cuda") -> cuda:<current>: the cached weights and plans compare devices, and "cuda" != "cuda:0"."""
    dev = torch.device(dev)
    return torch.device(dev.type, torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev


def _strip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    if sd and all(k.startswith("module.") for k in sd):
        return {k[len("module."):]: v for k, v in sd.items()}
    return sd


# ------------------------------------------------------------------------------------------------ weight packing
def _fold(bn: nn.BatchNorm2d):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.detach().double() * s


class _Packer:
    """Packs folded weights into one fp32 device buffer; every piece starts on a 16-float boundary.  With a 16-bit ``dtype`` the
    pointwise weights go into a second buffer of that type, in the layout of stl_det_pointwise16.  ``transposed`` (16-bit only, the
    heads of a model that trains): every pointwise layer also gets the bf16 transposed pack of stl_det_pointwise16_bwd_data, in a
    buffer of its own; ``tmap`` maps the forward pack's offset to (offset, Kp, Np) of the transposed one."""

    def __init__(self, dtype: torch.dtype = torch.float32, transposed: bool = False):
        self.parts, self.n = [], 0
        self.dtype, self.parts16, self.n16 = dtype, [], 0
        self.transposed, self.partsT, self.nT, self.tmap = transposed, [], 0, {}

    def add(self, t: torch.Tensor) -> int:
        off = self.n
        flat = t.reshape(-1).double()
        pad = (-flat.numel()) % 16
        self.parts.append(torch.cat([flat, flat.new_zeros(pad)]) if pad else flat)
        self.n += flat.numel() + pad
        return off

    def pw(self, conv: nn.Conv2d, bn: Optional[nn.BatchNorm2d] = None):
        """1x1 conv (+ BN) -> (w offset, bias offset or None, Kp, Np): w packed [Kp][Np] zero-padded, bias [Np].  16-bit: the w
        offset is into the 16-bit buffer, w rounded once from the fp64 fold and packed [Np / 16][Kp / 32][4][16][8] (a lane of the
        MFMA loads its 8 k of one column in 16 bytes), Kp % 32 == 0."""
        w = conv.weight.detach().double().reshape(conv.out_channels, conv.in_channels)
        b = conv.bias.detach().double() if conv.bias is not None else None
        if bn is not None:
            s, t = _fold(bn)
            w = w * s[:, None]
            b = t if b is None else b * s + t
        co, ci = w.shape
        h16 = self.dtype != torch.float32
        kp, np_ = -(-ci // 32) * 32 if h16 else -(-ci // 16) * 16, -(-co // 64) * 64
        bo = None if b is None else self.add(_padded(b[None], 1, np_))
        if not h16:
            return self.add(_padded(w.t(), kp, np_)), bo, kp, np_
        off, wp = self.n16, _tiles(_padded(w, np_, kp), self.dtype)
        self.parts16.append(wp)
        self.n16 += wp.numel()
        if self.transposed:
            wt, kt, nt = pack_transposed(w)
            self.tmap[off] = (self.nT, kt, nt)
            self.partsT.append(wt)
            self.nT += wt.numel()
        return off, bo, kp, np_

    def dw(self, conv: nn.Conv2d, bn: Optional[nn.BatchNorm2d] = None):
        """depthwise k x k (+ BN) -> (w offset [k][k][C], bias offset or None)."""
        w = conv.weight.detach().double()[:, 0]   # [C, k, k]
        bo = None
        if bn is not None:
            s, t = _fold(bn)
            w = w * s[:, None, None]
            bo = self.add(t)
        return self.add(w.permute(1, 2, 0).contiguous()), bo

    def done(self, dev) -> torch.Tensor:
        return torch.cat(self.parts).float().to(dev).contiguous() if self.parts else torch.zeros(1, device=dev)

    def done16(self, dev) -> Optional[torch.Tensor]:
        return torch.cat(self.parts16).to(dev).contiguous() if self.parts16 else None


def _padded(w: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """The matrix w in the top left corner of zeros [rows, cols]."""
    out = w.new_zeros(rows, cols)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _tiles(wp: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[Np, Kp] (n the output channel, k the contraction) -> flat [Np / 16][Kp / 32][4][16][8], the order of the 16-bit MFMA
    pointwise kernels (a lane loads its 8 k of one column in 16 bytes), rounded once to `dtype`."""
    np_, kp = wp.shape
    return wp.reshape(np_ // 16, 16, kp // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1).to(dtype)


def pack_transposed(w: torch.Tensor):
    """The folded fp64 W' [co, ci] -> (bf16 pack, Kp, Np) for the data gradient dX = dY W'^T: the forward's tile layout with the
    roles of k and n swapped (the contraction runs over co, padded to Kp % 32 == 0; the output over ci, padded to Np % 64 == 0),
    rounded once from the fp64 fold."""
    co, ci = w.shape
    kp, np_ = -(-co // 32) * 32, -(-ci // 64) * 64
    return _tiles(_padded(w.t(), np_, kp), torch.bfloat16), kp, np_


def unpack_transposed(wt: torch.Tensor, ci: int, co: int) -> torch.Tensor:
    """pack_transposed's inverse (``_tiles`` undone): the bf16 W'^T [ci, co]."""
    kp, np_ = -(-co // 32) * 32, -(-ci // 64) * 64
    return wt.reshape(np_ // 16, kp // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(np_, kp)[:ci, :co]


# ------------------------------------------------------------------------------------------------ the launch plan
def list_stem(ops: LaunchList, code: int, canvas, w, bias, out, B, H, W, co) -> None:
    """The stem (3x3 / 2 conv + BN + swish) of the fp32 H x W canvas onto `out`, stored in the type of `code`."""
    if code:
        ops.add("stl_det_stem16", code, canvas, w, bias, out, B, H, W, co)
    else:
        ops.add("stl_det_stem", canvas, w, bias, out, B, H, W, co)


def list_dwconv(ops: LaunchList, code: int, x, w, bias, y, B, h, c, k, s, act, partial=None) -> None:
    """Depthwise k x k / s on the h x h map x -> y; 16-bit with ``partial``: also the squeeze-excitation pooling sums."""
    if code:
        ops.add("stl_det_dwconv16", code, x, w, bias, y, partial, B, h, h, c, k, s, act)
    else:
        ops.add("stl_det_dwconv", x, w, bias, y, B, h, h, c, k, s, act)


def list_se(ops: LaunchList, code: int, x, part, nparts, B, hw, c, cse, w, scale) -> None:
    """Squeeze-excitation gate ``scale`` [B, c] of the map x; w: its four weight pieces.  fp32 pools x itself, with `part` as
    workspace (two launches); 16-bit reads the `nparts` pooling sums per image that the depthwise launch left in `part`."""
    if code:
        ops.add("stl_det_se16", part, B, hw, nparts, c, cse, *w, scale)
    else:
        ops.add("stl_det_se", x, B, hw, c, cse, *w, part, scale)


def list_pointwise(ops: LaunchList, code: int, fields, out_f32, z=None) -> None:
    """The 1x1 conv described by `fields` (``_Plan.pw_fields``); out_f32 (16-bit only): the output is fp32, not the type of `code`; z: the
    training entry point, which also stores the pre-activation there."""
    if code:
        p, name, train = capi.DetPointwise16(*fields, code, int(out_f32)), "stl_det_pointwise16", "stl_det_pointwise16_train"
    else:
        p, name, train = capi.DetPointwise(*fields), "stl_det_pointwise", "stl_det_pointwise_train"
    ops.add(*((name, p) if z is None else (train, p, z)))


def list_fuse(ops: LaunchList, code: int, out, terms, wparam):
    """The BiFPN node `out` [B, H, W, C] = fast-normalised sum of terms [(map, mode)] (wparam None: a plain resample).  Returns the
    listed descriptor."""
    f = capi.DetFuse()
    f.B, f.H, f.W, f.C, f.nterms = out.shape[0], out.shape[1], out.shape[2], out.shape[3], len(terms)
    for i, (t, mode) in enumerate(terms):
        f.t[i] = capi.DetTerm(t.data_ptr(), mode, t.shape[1], t.shape[2], 0)
    f.wparam = None if wparam is None else wparam.data_ptr()
    f.out = out.data_ptr()
    ops.keep_alive(out, *[t for t, _ in terms])   # the descriptor holds their addresses
    if code:
        ops.add("stl_det_fuse16", f, code)
    else:
        ops.add("stl_det_fuse", f)
    return f


# What the training backward (detector_train) reads of the forward, as _Plan keeps it.  blocks[i], an MBConv block: its input, the
# expand layer's output (None in a block without one), the depthwise layer's output, the squeeze-excitation gate [B, mid], its output;
# cells[j][node], a BiFPN node: the fused map, the depthwise layer's output, the node's output, the listed DetFuse, the maps it fuses;
# first_convs[name], one of the first cell's six 1x1 layers: the backbone map it reads, its output, its pack (w, bias, Kp, Np);
# first_pools, the first cell's two plain pools in forward order: the listed DetFuse, input, output
_T = torch.Tensor
BlockMaps = NamedTuple("BlockMaps", [("inp", _T), ("e", Optional[_T]), ("a", _T), ("gate", _T), ("y", _T)])
NodeMaps = NamedTuple("NodeMaps", [("f", _T), ("d", _T), ("y", _T), ("desc", ctypes.Structure), ("terms", List[_T])])
FirstConv = NamedTuple("FirstConv", [("x", _T), ("y", _T), ("pk", tuple)])
FirstPool = NamedTuple("FirstPool", [("desc", ctypes.Structure), ("x", _T), ("y", _T)])


class _Plan:
    """Every launch of one forward at batch B on the 512 canvas, with its buffers: ``calls``, a LaunchList replayed by
    ``run``; ``canvas`` is the input, ``feats`` the five BiFPN outputs (NHWC), ``reg`` / ``cls`` the head outputs.  In a 16-bit
    mode every activation buffer has the model's compute type and the *16 entry points are listed; canvas, reg and cls are fp32.
    ``launches`` counts kernel launches (the fp32 squeeze-excitation entry point is two: its pooling pass and the gate)."""

    def __init__(self, m: "EfficientDetBackbone", B: int, dev):
        self.B, self.dev, self.calls = B, dev, LaunchList()
        self._keep = self.calls.keep
        self.flops = self.bytes = self.launches = 0   # from the shapes: multiply-adds x 2, and every tensor each launch reads or writes once
        self.wbuf, self.wbuf16 = m._wbuf, m._wbuf16
        self.adtype, self.code = COMPUTE_DTYPES[m.compute_dtype]
        self.h16 = self.code != 0
        self.es = capi.DTYPES[self.code][0]   # bytes per stored activation / pointwise weight
        S = MAX_SIZE
        self.canvas = torch.empty(B, S, S, 3, device=dev)
        L = m._layout
        net = m.backbone_net.model
        H = (S + 1) // 2
        x = self._buf(B, H, H, net._conv_stem.conv.out_channels)
        list_stem(self.calls, self.code, self.canvas, self._w(L["stem"][0]), self._w(L["stem"][1]), x, B, S, S, x.shape[3])
        self._cost(2 * x.numel() * 27, 4 * self.canvas.numel() + self.es * x.numel())
        h = H
        feats, specs = [], net.specs
        self.blocks: List[BlockMaps] = []   # per MBConv block: the blocks' backward reads them
        for i, (b, lay) in enumerate(zip(specs, L["blocks"])):
            if b["s"] == 2:   # the wrapper keeps the input of every stride-2 block (efficientdet_utils/model.py:413-414)
                feats.append((x, h))
            inp = x
            if b["e"] != 1:
                y = self._buf(B, h, h, b["mid"])
                self._pw(x, y, h * h, b["ci"], b["mid"], lay["expand"], act=1)
                x = y
            e = x if b["e"] != 1 else None
            ho = (h + b["s"] - 1) // b["s"]
            y = self._buf(B, ho, ho, b["mid"])
            scale = torch.empty(B, b["mid"], device=dev)
            se = [self._w(o) for o in lay["se"]]
            if self.h16:   # the depthwise kernel writes the pooling sums: no pass over its output
                nparts = capi.lib().stl_det_dw16_parts(ho * ho)
                part = torch.empty(B * nparts * b["mid"], device=dev)
                self._dw(x, y, lay["dw"][0], lay["dw"][1], h, b["mid"], b["k"], b["s"], 1, part)
                h, x = ho, y
                list_se(self.calls, self.code, x, part, nparts, B, h * h, b["mid"], b["se"], se, scale)
                self._cost(part.numel() + 4 * B * b["mid"] * b["se"], 4 * part.numel())
            else:
                self._dw(x, y, lay["dw"][0], lay["dw"][1], h, b["mid"], b["k"], b["s"], 1)
                h, x = ho, y
                part = torch.empty(capi.lib().stl_det_se_workspace(B) * b["mid"], device=dev)
                list_se(self.calls, self.code, x, part, 0, B, h * h, b["mid"], b["se"], se, scale)
                self._cost(x.numel() + 4 * B * b["mid"] * b["se"], 4 * x.numel(), launches=2)
            y = self._buf(B, h, h, b["co"])
            self._pw(x, y, h * h, b["mid"], b["co"], lay["project"], act=0, in_scale=scale, residual=inp if b["skip"] else None)
            self.blocks.append(BlockMaps(inp, e, x, scale, y))
            x = y
        feats.append((x, h))
        p3, p4, p5 = feats[-3:]
        self.backbone = [f for f, _ in feats[-3:]]   # P3, P4, P5
        c = m.fpn_channels
        levels = None
        self.cells: List[Dict[str, NodeMaps]] = []   # per BiFPN cell {node: its maps}: the cells' backward reads them
        for cell, lay in zip(m.bifpn, L["bifpn"]):
            levels = self._bifpn(cell, lay, levels, p3, p4, p5, c)
        self.feats = levels
        A, nc = m.num_anchors_total, m.num_classes
        self.head_start = len(self.calls)   # calls[:head_start] is the frozen trunk (detector_train runs the heads itself)
        self.train = None                   # detector_train.HeadTrain, built by the first detection_loss of this batch size
        self.reg = torch.empty(B, A, 4, device=dev)
        self.cls = torch.empty(B, A, nc, device=dev)
        for head, lay, out, k, act in ((m.regressor, L["regressor"], self.reg, 4, 0), (m.classifier, L["classifier"], self.cls, nc, 2)):
            aoff = 0
            for li, (f, hh) in enumerate(levels):
                t = f
                for i in range(len(head.conv_list)):
                    d = self._buf(B, hh, hh, c)
                    self._dw(t, d, lay["dw"][i], None, hh, c, 3, 1, 0)
                    e = self._buf(B, hh, hh, c)
                    self._pw(d, e, hh * hh, c, c, lay["pw"][li][i], act=1)
                    t = e
                d = self._buf(B, hh, hh, c)
                self._dw(t, d, lay["hdw"], None, hh, c, 3, 1, 0)
                self._pw(d, out, hh * hh, c, 9 * k, lay["hpw"], act=act, img_stride=A * k, row_stride=9 * k, off=aoff * k)
                aoff += hh * hh * 9

    def _buf(self, B, h, w, c):
        return torch.empty(B, h, w, c, device=self.dev, dtype=self.adtype)

    def _w(self, off):
        return None if off is None else self.wbuf[off:]

    def _cost(self, flops, nbytes, launches=1):
        """Count the entry just listed."""
        self.flops += int(flops)
        self.bytes += int(nbytes)
        self.launches += launches

    def _dw(self, x, y, w, bias, h, c, k, s, act, partial=None):
        list_dwconv(self.calls, self.code, x, self._w(w), self._w(bias), y, self.B, h, c, k, s, act, partial)
        self._cost(2 * y.numel() * k * k, self.es * (x.numel() + y.numel()) + (0 if partial is None else 4 * partial.numel()))

    def pw_fields(self, x, out, hw, ci, co, pk, act, in_scale=None, residual=None, img_stride=None, row_stride=None, off=0):
        """The fields of capi.DetPointwise, which DetPointwise16 starts with too, for the layer packed as pk = (w, bias, Kp, Np) in
        this plan's weight buffers: the B x hw rows of ci channels onto co, written densely unless the strides and the offset
        place them inside a larger output.  The tensors are the caller's to keep."""
        w, b, kp, np_ = pk
        ptrs = [None if t is None else t.data_ptr() for t in (x, (self.wbuf16 if self.h16 else self.wbuf)[w:], self._w(b), in_scale, residual, out)]
        return (*ptrs, self.B * hw, hw * co if img_stride is None else img_stride, co if row_stride is None else row_stride, off, hw,
                ci, co, kp, np_, act)

    def _pw(self, x, out, hw, ci, co, pk, act, in_scale=None, residual=None, **place):
        m, (_, _, kp, np_) = self.B * hw, pk
        self.calls.keep_alive(x, out, in_scale, residual)   # the descriptor holds their addresses
        list_pointwise(self.calls, self.code, self.pw_fields(x, out, hw, ci, co, pk, act, in_scale, residual, **place),
                       out.dtype == torch.float32)
        self._cost(2 * m * ci * co, self.es * (m * ci + kp * np_ + (m * co if residual is not None else 0)) + out.element_size() * m * co)

    def _fuse(self, out, terms, wparam):
        f = list_fuse(self.calls, self.code, out, terms, wparam)
        self._cost(out.numel() * (2 * len(terms) + 4), self.es * (out.numel() + sum(t.numel() for t, _ in terms)))
        return f

    def _sep(self, x, pk, h, c):
        """SeparableConvBlock: depthwise 3x3 (no bias) then 1x1 with bias and BN folded, no activation -> (depthwise output, output)."""
        d = self._buf(self.B, h, h, c)
        self._dw(x, d, pk[0], None, h, c, 3, 1, 0)
        y = self._buf(self.B, h, h, c)
        self._pw(d, y, h * h, c, c, pk[1], act=0)
        return d, y

    def _bifpn(self, cell, lay, levels, p3, p4, p5, c):
        B = self.B
        wp = lay["weights"]
        if levels is None:
            (x3, h3), (x4, h4), (x5, h5) = p3, p4, p5
            t = self._buf(B, h5, h5, c)
            self._pw(x5, t, h5 * h5, x5.shape[3], c, lay["p5_to_p6"], act=0)
            h6, h7 = (h5 + 1) // 2, (h5 + 3) // 4
            p6 = self._buf(B, h6, h6, c)
            p7 = self._buf(B, h7, h7, c)
            # what the first cell's backward reads: its two plain pools in forward order and its six 1x1 layers by name
            self.first_pools = [FirstPool(self._fuse(p6, [(t, 2)], None), t, p6), FirstPool(self._fuse(p7, [(p6, 2)], None), p6, p7)]
            self.first_convs = {"p5_to_p6": FirstConv(x5, t, lay["p5_to_p6"])}
            ins = []
            for (xx, hh), key in ((p3, "p3_down_channel"), (p4, "p4_down_channel"), (p5, "p5_down_channel")):
                y = self._buf(B, hh, hh, c)
                self._pw(xx, y, hh * hh, xx.shape[3], c, lay[key], act=0)
                self.first_convs[key] = FirstConv(xx, y, lay[key])
                ins.append(y)
            p3_in, p4_in, p5_in = ins
            p6_in, p7_in = p6, p7
        else:
            (p3_in, _), (p4_in, _), (p5_in, _), (p6_in, _), (p7_in, _) = levels
        hs = [p.shape[1] for p in (p3_in, p4_in, p5_in, p6_in, p7_in)]

        kept = {}
        self.cells.append(kept)

        def node(name, wname, terms, h):
            f = self._buf(B, h, h, c)
            desc = self._fuse(f, terms, wp[wname])
            d, y = self._sep(f, lay[name], h, c)
            kept[name] = NodeMaps(f, d, y, desc, [t for t, _ in terms])
            return y
        p6_up = node("conv6_up", "p6_w1", [(p6_in, 0), (p7_in, 1)], hs[3])
        p5_up = node("conv5_up", "p5_w1", [(p5_in, 0), (p6_up, 1)], hs[2])
        p4_up = node("conv4_up", "p4_w1", [(p4_in, 0), (p5_up, 1)], hs[1])
        p3_out = node("conv3_up", "p3_w1", [(p3_in, 0), (p4_up, 1)], hs[0])
        if levels is None:
            ins = []
            for (xx, hh), key in ((p4, "p4_down_channel_2"), (p5, "p5_down_channel_2")):
                y = self._buf(B, hh, hh, c)
                self._pw(xx, y, hh * hh, xx.shape[3], c, lay[key], act=0)
                self.first_convs[key] = FirstConv(xx, y, lay[key])
                ins.append(y)
            p4_in, p5_in = ins
        p4_out = node("conv4_down", "p4_w2", [(p4_in, 0), (p4_up, 0), (p3_out, 2)], hs[1])
        p5_out = node("conv5_down", "p5_w2", [(p5_in, 0), (p5_up, 0), (p4_out, 2)], hs[2])
        p6_out = node("conv6_down", "p6_w2", [(p6_in, 0), (p6_up, 0), (p5_out, 2)], hs[3])
        p7_out = node("conv7_down", "p7_w2", [(p7_in, 0), (p6_out, 2)], hs[4])
        return [(p, p.shape[1]) for p in (p3_out, p4_out, p5_out, p6_out, p7_out)]

    def run(self, stream: int, upto: Optional[int] = None, canvas: Optional[torch.Tensor] = None) -> None:
        """canvas: another fp32 [B, S, S, 3] input than the plan's own (a ``DetBatch``'s): the stem, the first launch and the canvas's
        only reader, reads it where it lies -- nothing is copied."""
        if self.train is not None:
            self.train.generation += 1   # the maps a pending backward would read are about to be overwritten
        if canvas is None or canvas.data_ptr() == self.canvas.data_ptr():
            return self.calls.run(stream, 0, upto)
        if tuple(canvas.shape) != tuple(self.canvas.shape) or canvas.dtype != torch.float32 or canvas.device != self.canvas.device \
                or not canvas.is_contiguous():
            raise ValueError(f"EfficientDet: the batch's canvas must be contiguous float32 {tuple(self.canvas.shape)} on {self.canvas.device}, "
                             f"got {canvas.dtype} {tuple(canvas.shape)} on {canvas.device}")
        fn, name, args = self.calls.calls[0]
        own = self.canvas.data_ptr()
        mine = [isinstance(a, ctypes.c_void_p) and a.value == own for a in args]
        assert name in ("stl_det_stem", "stl_det_stem16") and sum(mine) == 1, "EfficientDet: the plan's first launch is not the stem"
        args = tuple(ctypes.c_void_p(canvas.data_ptr()) if m else a for a, m in zip(args, mine))
        capi.check(fn(*args, ctypes.c_void_p(stream)), name)
        self.calls.run(stream, 1, upto)


# ------------------------------------------------------------------------------------------------ the model
class EfficientDetBackbone(nn.Module):
    """models.EfficientDet (EfficientDetBackbone, src/models/EfficientDet.py:16-133) on the MI355X: inference (forward) and
    fine-tuning of the heads (detection_loss).

    forward(inputs, preprocess=True, postprocess=True, threshold=None, iou_threshold=None): inputs a float tensor [B, 3, H, W]
    (04 passes ``img / 255``) or a list of CHW float arrays in [0, 1]; postprocess=False returns (features, regression,
    classification, anchors) with the reference's shapes (five NCHW maps, [B, A, 4], [B, A, num_classes] after the sigmoid,
    [1, A, 4]) on the GPU; otherwise one dict per image with CPU tensors ``boxes`` float32 [k, 4] (x1, y1, x2, y2 in original
    pixels), ``labels`` int32 (class + 1) and ``scores`` float32, in NMS keep order.  Raises in training mode.

    compute_dtype "fp32" (default), "bf16" or "f16": the type the activations are stored in on the device (module docstring);
    the outputs are fp32 in every mode.  A model keeps its compute_dtype for life."""

    def __init__(self, num_classes=80, compound_coef=0, load_weights=False, compute_dtype="fp32", **kwargs):
        super().__init__()
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError(f"EfficientDet: compute_dtype {compute_dtype!r} (one of 'fp32', 'bf16', 'f16')")
        self.compute_dtype = compute_dtype
        if compound_coef not in FPN_FILTERS:
            raise NotImplementedError(f"EfficientDet: compound_coef {compound_coef} (supported: 0 and 3, what setup_detector allows)")
        if load_weights:
            raise NotImplementedError("EfficientDet: load_weights=True downloads pretrained EfficientNet weights; load a state_dict")
        if int(num_classes) < 1:
            raise ValueError(f"EfficientDet: num_classes = {num_classes}")
        self.compound_coef = cc = compound_coef
        ratios = kwargs.get("ratios", RATIOS)
        scales = kwargs.get("scales", SCALES)
        if [tuple(r) for r in ratios] != RATIOS or len(scales) != 3 or not np.allclose(scales, SCALES):
            raise NotImplementedError("EfficientDet: only the reference's anchor ratios and scales are supported")
        self.num_classes = int(num_classes)
        self.fpn_channels = c = FPN_FILTERS[cc]
        self.bifpn = nn.Sequential(*[_BiFPN(c, P345_CHANNELS[cc], i == 0) for i in range(FPN_REPEATS[cc])])
        self.regressor = _Head(c, 9 * 4, HEAD_REPEATS[cc])
        self.classifier = _Head(c, 9 * self.num_classes, HEAD_REPEATS[cc])
        self.backbone_net = _Backbone(cc)
        self.threshold = kwargs.get("threshold", 0.6)
        self.iou_threshold = kwargs.get("iou_threshold", 0.5)
        self.anchors_np = anchors(cc)
        self.num_anchors_total = self.anchors_np.shape[0]
        self._version, self._plans, self._wbuf, self._wbuf16, self._anchor_dev = None, {}, None, None, None
        self._wbufT16, self._layoutT = None, None   # the heads' bf16 transposed packs (_ensure_transposed: models that train only)
        self._batch_tables: dict = {}               # _batch_records: the constant record table of a DetBatch geometry
        self.train_bifpn = 0                        # set_train_bifpn: how many trailing BiFPN cells detection_loss trains with the heads ("all": every cell)
        self.train_backbone = 0                     # set_train_backbone / set_train_trunk: how many trailing MBConv blocks train with them
        self.train_stem = False                     # set_train_trunk("all"): the stem (_conv_stem, _bn0) trains too, with every block
        self.eval()

    # ---------------------------------------------------------------- state
    def load_state_dict(self, state_dict, strict=True, assign=False):
        return super().load_state_dict(_strip(dict(state_dict)), strict=strict, assign=assign)

    def set_train_bifpn(self, k) -> "EfficientDetBackbone":
        """The last k BiFPN cells train with the heads in detection_loss (0: the heads alone), k = 0 .. cells - 1; ``"all"``: every
        cell, the first one included (``train_bifpn == len(bifpn)``).  The first cell does not train by count: it alone has the
        down-channel convs, p5_to_p6 and the unweighted pooled maps, where the frozen backbone's P3 / P4 / P5 enter the pyramid,
        and with it trains everything behind the backbone; the backbone stays frozen and gets no data gradient."""
        n = len(self.bifpn)
        if isinstance(k, str) and k == "all":
            k = n
        elif not isinstance(k, int) or isinstance(k, bool) or k < 0 or k > n - 1:
            raise ValueError(f"EfficientDet.set_train_bifpn: k = {k!r}, expected 0 .. {n - 1}: the first of the {n} BiFPN cells does not "
                             "train by count -- it alone has the down-channel convs, p5_to_p6 and the unweighted pooled maps; "
                             "set_train_bifpn(\"all\") trains it with every cell behind it")
        if (self.train_backbone or self.train_stem) and k != n:
            raise ValueError(f"EfficientDet.set_train_bifpn: {self.train_backbone} backbone block(s) train, which needs every BiFPN cell to "
                             "train (the gradient of P5 exists only when the first cell trains): call set_train_backbone(0) first")
        if k != self.train_bifpn:
            current = self._version is not None and self._state_version() == self._version
            self.train_bifpn = k
            self._version = self._state_version() if current else None   # the same weights, split anew; else a full refold
            for p in self._plans.values():
                p.train = None   # its backward launches are listed for one k
        return self

    def final_stage_blocks(self) -> int:
        """The number of MBConv blocks of the backbone's final stage, the ones that produce P5 (from ``block_specs``: the trailing
        expanding blocks whose depthwise layer is 3 x 3, stride 1 -- what the blocks' backward covers)."""
        specs, n = self.backbone_net.model.specs, 0
        while n < len(specs) and specs[-1 - n]["k"] == 3 and specs[-1 - n]["s"] == 1 and specs[-1 - n]["e"] != 1:
            n += 1
        return n

    def set_train_backbone(self, k) -> "EfficientDetBackbone":
        """The last k MBConv blocks of the backbone train with the BiFPN and the heads in detection_loss (0: none), k = 0 .. the
        blocks of the final stage (1 for D0, 2 for D3), the ones that produce P5.  Needs ``set_train_bifpn("all")``: the gradient of
        P5 exists only when the first cell trains.  fp32 only; every BN stays on its running statistics; drop-connect is not
        applied (the training forward is the inference forward)."""
        n = self.final_stage_blocks()
        if not isinstance(k, int) or isinstance(k, bool) or k < 0:
            raise ValueError(f"EfficientDet.set_train_backbone: k = {k!r}, expected 0 .. {n}")
        if k > n:
            raise ValueError(f"EfficientDet.set_train_backbone: k = {k!r}, expected 0 .. {n}: only the {n} block(s) of the backbone's final "
                             "stage train -- the blocks in front have 5x5 / stride-2 depthwise layers whose backward does not exist yet "
                             "in this setter's contract; set_train_trunk(k) reaches them (any block, \"all\": the stem too)")
        return self._set_trunk("set_train_backbone", k, False)

    def set_train_trunk(self, k) -> "EfficientDetBackbone":
        """``set_train_backbone`` without the final stage's limit: the last k MBConv blocks of the whole backbone train, k = 0 .. the
        number of blocks (16 for D0, 26 for D3) -- the 5 x 5 and stride-2 depthwise layers and the blocks without an expand layer among
        them (csrc/detector_trunk.hip); ``"all"``: every block and the stem (``_conv_stem``, ``_bn0``; ``train_stem``).  The count goes to
        ``train_backbone``; up to ``final_stage_blocks()`` the two setters do the same.  The same preconditions and contract: needs
        ``set_train_bifpn("all")``, fp32 only, every BN on its running statistics, no drop-connect, the forward launch list unchanged."""
        n = len(self.backbone_net.model._blocks)
        stem = isinstance(k, str) and k == "all"
        if stem:
            k = n
        elif not isinstance(k, int) or isinstance(k, bool) or k < 0 or k > n:
            raise ValueError(f"EfficientDet.set_train_trunk: k = {k!r}, expected 0 .. {n} (the last k MBConv blocks) or \"all\" (every block "
                             "and the stem)")
        return self._set_trunk("set_train_trunk", k, stem)

    def _set_trunk(self, who: str, k: int, stem: bool) -> "EfficientDetBackbone":
        if k and self.train_bifpn != len(self.bifpn):
            raise ValueError(f"EfficientDet.{who}: the gradient of P5 exists only when the first BiFPN cell trains: call "
                             "set_train_bifpn(\"all\") first")
        if k != self.train_backbone or stem != self.train_stem:
            current = self._version is not None and self._state_version() == self._version
            self.train_backbone, self.train_stem = k, stem
            self._version = self._state_version() if current else None   # the same weights, split anew; else a full refold
            for p in self._plans.values():
                p.train = None   # its backward launches are listed for one k
        return self

    def _state_version(self):
        """(trunk, blocks, cells, heads): data pointer and version of every parameter and buffer of the frozen trunk, of the trainable
        MBConv blocks (the last train_backbone), of the trainable BiFPN cells (the last train_bifpn) and of regressor.* / classifier.*"""
        owned = lambda mods: [t for h in mods for t in list(h.parameters()) + list(h.buffers())]   # noqa: E731
        allb = list(self.backbone_net.model._blocks)
        net = self.backbone_net.model
        blocks = owned(([net._conv_stem, net._bn0] if self.train_stem else []) + allb[len(allb) - self.train_backbone:])   # the stem with them
        cells = owned(list(self.bifpn)[len(self.bifpn) - self.train_bifpn:])
        heads = owned((self.regressor, self.classifier))
        ids = {id(t) for t in blocks + cells + heads}
        trunk = [t for t in list(self.parameters()) + list(self.buffers()) if id(t) not in ids]
        return tuple(tuple((t.data_ptr(), t._version) for t in ts) for ts in (trunk, blocks, cells, heads))

    def _pack_stem(self, P: _Packer):
        """-> (w offset [3][3][3][Co], bias offset) of the stem with its BN folded"""
        net = self.backbone_net.model
        s, t = _fold(net._bn0)
        return (P.add((net._conv_stem.conv.weight.detach().double() * s[:, None, None, None]).permute(2, 3, 1, 0).contiguous()), P.add(t))

    @staticmethod
    def _pack_block(P: _Packer, blk, b) -> dict:
        lay = {"dw": P.dw(blk._depthwise_conv.conv, blk._bn1), "project": P.pw(blk._project_conv.conv, blk._bn2)}
        if b["e"] != 1:
            lay["expand"] = P.pw(blk._expand_conv.conv, blk._bn0)
        r, e = blk._se_reduce.conv, blk._se_expand.conv
        lay["se"] = (P.add(r.weight.detach().reshape(b["se"], b["mid"])), P.add(r.bias.detach()),
                     P.add(e.weight.detach().reshape(b["mid"], b["se"])), P.add(e.bias.detach()))
        return lay

    @staticmethod
    def _pack_cell(P: _Packer, cell):
        """-> (the packed layers' offsets by name, the fusion weights' offsets by name)"""
        lay = {}
        for n in _BiFPN.NODES:
            sep = getattr(cell, n)
            lay[n] = (P.dw(sep.depthwise_conv.conv)[0], P.pw(sep.pointwise_conv.conv, sep.bn))
        if cell.first_time:
            for key in ("p5_down_channel", "p4_down_channel", "p3_down_channel", "p5_to_p6", "p4_down_channel_2", "p5_down_channel_2"):
                seq = getattr(cell, key)
                lay[key] = P.pw(seq[0].conv, seq[1])
        return lay, {n: P.add(getattr(cell, n).detach()) for n, _ in _BiFPN.WEIGHTS}

    def _pack_heads(self, P: _Packer) -> dict:
        heads = {}
        for name in ("regressor", "classifier"):
            hd = getattr(self, name)
            heads[name] = {"dw": [P.dw(cv.depthwise_conv.conv)[0] for cv in hd.conv_list],
                           "pw": [[P.pw(cv.pointwise_conv.conv, hd.bn_list[lv][i]) for i, cv in enumerate(hd.conv_list)] for lv in range(5)],
                           "hdw": P.dw(hd.header.depthwise_conv.conv)[0], "hpw": P.pw(hd.header.pointwise_conv.conv)}
        return heads

    def _refold_tail(self, first: int, block: Optional[int] = None) -> None:
        """Only the BiFPN cells from `first` on and regressor.* / classifier.* changed (an optimiser step of detection_loss; first =
        len(bifpn): the heads alone).  The cells are packed in order and the heads last, so these pieces are one tail of the weight
        buffers: it is rewritten in place, through the same packing as a full refold (bit-identical); the plans stay.  block: the
        MBConv blocks from that one on changed too (first = 0 then); they are packed in front of the cells: a longer tail."""
        P = _Packer(COMPUTE_DTYPES[self.compute_dtype][0])
        net = self.backbone_net.model
        n0, n16 = P.n, P.n16 = self._tail_off[first] if block is None else (0, 0) if block < 0 else self._block_off[block]
        if block is not None:
            assert first == 0, "EfficientDet: trainable blocks without every cell"
            if block < 0:   # the stem trains: it is packed first, so the tail is the whole buffer
                assert self._pack_stem(P) == self._layout["stem"] and (P.n, P.n16) == self._block_off[0], "EfficientDet: stem layout changed"
            for i in range(max(block, 0), len(net._blocks)):
                assert self._pack_block(P, net._blocks[i], net.specs[i]) == self._layout["blocks"][i], "EfficientDet: block layout changed"
            assert (P.n, P.n16) == self._tail_off[0], "EfficientDet: block layout changed"
        for j in range(first, len(self.bifpn)):
            lay, woff = self._pack_cell(P, self.bifpn[j])
            assert all(lay[k] == self._layout["bifpn"][j][k] for k in lay) and woff == self._woff[j], "EfficientDet: BiFPN layout changed"
        assert (P.n, P.n16) == self._tail_off[len(self.bifpn)], "EfficientDet: BiFPN layout changed"
        P.transposed = self._wbufT16 is not None   # the heads alone have transposed packs
        heads = self._pack_heads(P)
        assert all(heads[k] == self._layout[k] for k in heads) and P.n == self._wbuf.numel(), "EfficientDet: head layout changed"
        self._wbuf[n0:].copy_(torch.cat(P.parts).float())
        if P.parts16:
            self._wbuf16[n16:].copy_(torch.cat(P.parts16))
        if P.partsT:
            assert P.tmap == self._layoutT, "EfficientDet: head layout changed"
            self._wbufT16.copy_(torch.cat(P.partsT))

    def _ensure_transposed(self) -> None:
        """16-bit models that train: the bf16 transposed packs of the heads' pointwise layers (stl_det_pointwise16_bwd_data), built
        at the first detection_loss after a full fold and refreshed by _refold_tail; the forward buffers are not touched."""
        if self._wbufT16 is None:
            P = _Packer(COMPUTE_DTYPES[self.compute_dtype][0], transposed=True)
            P.n, P.n16 = self._tail_off[len(self.bifpn)]
            self._pack_heads(P)
            self._wbufT16, self._layoutT = torch.cat(P.partsT).to(self._wbuf.device).contiguous(), P.tmap

    def ready(self, dev) -> None:
        """Fold BN and pack every weight into one fp32 device buffer (in a 16-bit mode the pointwise weights into a second one of
        that type); redone when any parameter or buffer of the frozen trunk has changed (_refold_tail when only the trainable
        BiFPN cells' or the heads' have)."""
        dev = _device(dev)
        if self.backbone_net.model._bn0.weight.device != dev:
            self.to(dev)
        v = self._state_version()
        if self._version is not None and v[0] == self._version[0] and self._wbuf is not None and self._wbuf.device == dev:
            if v[1] != self._version[1]:   # the trainable blocks moved: with them every cell trains
                self._refold_tail(0, -1 if self.train_stem else len(self.backbone_net.model._blocks) - self.train_backbone)
            elif v[2:] != self._version[2:]:
                self._refold_tail(len(self.bifpn) - (self.train_bifpn if v[2] != self._version[2] else 0))
            self._version = v
            return
        P = _Packer(COMPUTE_DTYPES[self.compute_dtype][0])
        net = self.backbone_net.model
        stem = self._pack_stem(P)
        blocks, self._block_off = [], []   # _block_off[i]: where block i starts in the two buffers (the blocks in order, in front of the cells)
        for blk, b in zip(net._blocks, net.specs):
            self._block_off.append((P.n, P.n16))
            blocks.append(self._pack_block(P, blk, b))
        cells, self._woff, self._tail_off = [], [], []   # _tail_off[j]: where cell j starts in the two buffers, [len(bifpn)]: where the heads do
        for cell in self.bifpn:          # (cells in order, the heads last: _refold_tail rewrites the buffers from one of these on)
            self._tail_off.append((P.n, P.n16))
            lay, woff = self._pack_cell(P, cell)
            cells.append(lay)
            self._woff.append(woff)
        self._tail_off.append((P.n, P.n16))
        heads = self._pack_heads(P)
        self._wbuf, self._wbuf16 = P.done(dev), P.done16(dev)
        self._wbufT16, self._layoutT = None, None
        for cell, woff in zip(cells, self._woff):   # BiFPN weight offsets -> device views
            cell["weights"] = {n: self._wbuf[o:] for n, o in woff.items()}
        self._layout = {"stem": stem, "blocks": blocks, "bifpn": cells, **heads}
        self._anchor_dev = torch.from_numpy(self.anchors_np).to(dev)
        self._plans.clear()
        self._version = self._state_version()

    MAX_PLANS = 4   # plans own every intermediate (no buffer reuse): D3 at batch 32 holds several GB; least recently used go first

    def plan(self, B: int, dev) -> _Plan:
        dev = _device(dev)
        self.ready(dev)
        p = self._plans.pop(B, None)
        if p is None:
            while len(self._plans) >= self.MAX_PLANS:
                self._plans.pop(next(iter(self._plans)))
            p = _Plan(self, B, dev)
        self._plans[B] = p   # most recently used last
        return p

    # ---------------------------------------------------------------- forward
    def _check_mode(self):
        if self.training:
            raise NotImplementedError("EfficientDet runs in inference mode only (no backward, no training): call .eval() first")

    def _preprocess(self, srcs: List[torch.Tensor], kind: int, dev):
        """srcs on `dev`: kind 0 uint8 HWC, 1 float32 CHW.  Fills the plan's canvas; returns (plan, metas)."""
        B = len(srcs)
        p = self.plan(B, dev)
        recs = (capi.DetImage * B)()
        metas = []
        for i, s in enumerate(srcs):
            oh, ow = (s.shape[0], s.shape[1]) if kind == 0 else (s.shape[1], s.shape[2])
            m = resize_meta(int(oh), int(ow))
            metas.append(m)
            new_w, new_h = m[0], m[1]
            recs[i] = capi.DetImage(s.data_ptr(), kind, oh, ow, new_h, new_w, 0, 1.0 / (new_h / oh), 1.0 / (new_w / ow))
        tab = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(dev)
        capi.call("stl_det_preprocess", tab.data_ptr(), B, MAX_SIZE, p.canvas.data_ptr(), ops._st())
        return p, metas, (tab, srcs)

    def _float_sources(self, inputs, dev):
        if torch.is_tensor(inputs):
            if inputs.dim() != 4 or inputs.shape[1] != 3:
                raise ValueError(f"EfficientDet: inputs must be [B, 3, H, W], got {tuple(inputs.shape)}")
            x = inputs.detach().to(dev, torch.float32).contiguous()
            return [x[i] for i in range(x.shape[0])]
        out = []
        for a in inputs:
            t = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float32))
            if t.dim() != 3 or t.shape[0] != 3:
                raise ValueError(f"EfficientDet: each image must be CHW with 3 channels, got {tuple(t.shape)}")
            out.append(t.to(dev).contiguous())
        return out

    def run_raw(self, srcs, kind: int, dev):
        """Preprocess + network on `dev`; returns (plan, metas)."""
        self._check_mode()
        with torch.no_grad():
            p, metas, keep = self._preprocess(srcs, kind, dev)
            p.run(ops._st())
            self._range_guard(p)
        p._inflight = keep   # the sources and the record table live until the next call
        p._records = (metas, keep[0])   # output="device" divides by these records' ratios
        return p, metas

    def _batch_records(self, batch, dev):
        """(metas, device record table) of a ``DetBatch``: B times its constant ``resize_meta(S1, S1)``, built and uploaded once per
        (batch size, S1) and held: a batch builds no host table."""
        key = (len(batch), tuple(batch.meta), str(dev))
        held = self._batch_tables.get(key)
        if held is None:
            metas = [tuple(batch.meta)] * len(batch)
            held = self._batch_tables[key] = (metas, self._record_table(None, metas, dev))
        return held

    def run_batch(self, batch, dev):
        """run_raw for a ``det_data.DetBatch``: the network reads the batch's canvas where it lies; returns (plan, metas)."""
        self._check_mode()
        p = self.plan(len(batch), dev)
        with torch.no_grad():
            p.run(ops._st(), canvas=batch.canvas)
            self._range_guard(p)
        metas, table = self._batch_records(batch, dev)
        p._inflight = batch   # the canvas lives until the next call
        p._records = (metas, table)
        return p, metas

    def detection_loss(self, inputs, targets=None, alpha=0.25, gamma=2.0, box_weight=50.0) -> Dict[str, torch.Tensor]:
        """The fine-tuning counterpart of ``loss_dict = model(imgs / 255, targets)`` (02_train_faster_rcnn.py:212): the focal
        classification and smooth-L1 box regression losses of RetinaNet / EfficientDet over IoU-assigned anchors.  inputs as
        forward takes them; targets one dict per image with ``boxes`` [n, 4] (x1, y1, x2, y2 in original pixels) and ``labels``
        [n] in 1 .. num_classes (n = 0 allowed).  Returns {"classification", "regression"}: fp32 device scalars whose backward
        fills ``.grad`` of every regressor.* and classifier.* parameter and, after ``set_train_bifpn(k)``, of the last k BiFPN cells'
        (``"all"``: of every cell's; fp32 only) and, after ``set_train_backbone(k)``, of the backbone's last k MBConv blocks'; the rest of the backbone and the other cells are frozen and every BN runs on its running statistics, whatever ``.training`` is.  compute_dtype "fp32", or "f16" (f16 forward tensors, bf16 gradients in
        flight, fp32 sums and fp32 ``.grad``; non-finite head outputs raise FloatingPointError); "bf16" raises
        NotImplementedError.  One activation set per batch size: backward before the
        next detection_loss of that batch size (a stale-forward error otherwise).  See stlpose_amd/detector_train.py.

        ``detection_loss(batch)`` with a ``det_data.DetBatch`` (``DetBatchLoader``) and no targets: the network reads the batch's
        canvas and stl_det_loss its ``gt`` / ``offsets`` tables; nothing is copied and no host table is built."""
        from . import detector_train
        return detector_train.detection_loss(self, inputs, targets, alpha, gamma, box_weight)

    def _range_guard(self, p: _Plan) -> None:
        """f16 only: an activation past 65504 became inf and reaches the head outputs as inf or NaN (one small reduction)."""
        if self.compute_dtype == "f16" and not bool((torch.isfinite(p.reg).all() & torch.isfinite(p.cls).all()).item()):
            raise FloatingPointError("EfficientDet: non-finite head outputs in compute_dtype='f16': activations left f16's range "
                                     "(largest finite value 65504); build the detector with compute_dtype='bf16'")

    def forward(self, inputs, preprocess=True, postprocess=True, threshold=None, iou_threshold=None, output="host"):
        """output="host": the reference's list of per-image dicts of CPU tensors.  output="device": a ``detections.Detections``,
        the same detections as device tables from one launch, with no wait for the device (``.to_list()`` gives the list).
        inputs may be a ``det_data.DetBatch``: its canvas is the network's input as it lies, and the boxes come back on the scale of
        its S1 x S1 images."""
        self._check_mode()
        _check_output(output)
        if threshold is not None:
            self.threshold = threshold
        if iou_threshold is not None:
            self.iou_threshold = iou_threshold
        dev = torch.device("cuda", torch.cuda.current_device())
        if _is_det_batch(inputs):   # a det_data.DetBatch is preprocessed already, whatever `preprocess` says
            p, metas = self.run_batch(inputs, _device(inputs.canvas.device))
        elif preprocess:
            p, metas = self.run_raw(self._float_sources(inputs, dev), 1, dev)
        else:
            x = inputs.detach().to(dev, torch.float32)
            if tuple(x.shape[1:]) != (3, MAX_SIZE, MAX_SIZE):
                raise ValueError(f"EfficientDet: preprocess=False takes [B, 3, {MAX_SIZE}, {MAX_SIZE}], got {tuple(x.shape)}")
            p = self.plan(x.shape[0], dev)
            with torch.no_grad():
                p.canvas.copy_(x.permute(0, 2, 3, 1))
                p.run(ops._st())
                self._range_guard(p)
            metas = None
        if not postprocess:
            feats = tuple(f.permute(0, 3, 1, 2).to(torch.float32, copy=True) for f, _ in p.feats)
            return feats, p.reg.clone(), p.cls.clone(), self._anchor_dev[None].clone()
        return self.detect(p, metas, self.threshold, self.iou_threshold, output)

    def detect(self, p: _Plan, metas, threshold, iou_threshold, output="host"):
        """postprocess + invert_affine + the reference's dict format from a plan's head outputs; output="device": the same as a
        ``Detections`` (one launch, nothing copied)."""
        if _check_output(output) == "device":
            return detect_on_device(p.reg, p.cls, self._anchor_dev, threshold, iou_threshold, self._record_table(p, metas))
        dets = detect_from_heads(p.reg, p.cls, self._anchor_dev, threshold, iou_threshold)
        out = []
        for i, (boxes, cls, scores) in enumerate(dets):
            if len(scores) == 0:
                out.append({"boxes": torch.zeros(0), "labels": torch.zeros(0, dtype=torch.int32), "scores": torch.zeros(0)})
                continue
            if metas is not None:
                boxes = invert_affine(metas[i], boxes)
            out.append({"boxes": torch.from_numpy(boxes), "labels": torch.from_numpy(cls.astype(np.int32)) + 1,
                        "scores": torch.from_numpy(scores)})
        return out

    def _record_table(self, p: Optional[_Plan], metas, dev=None) -> Optional[torch.Tensor]:
        """The device table of StlDetImage records that belongs to `metas`: the one run_raw uploaded, or a new upload."""
        if metas is None:
            return None
        held = getattr(p, "_records", None)
        if held is not None and held[0] is metas:
            return held[1]
        recs = (capi.DetImage * len(metas))()
        for i, (new_w, new_h, old_w, old_h, *_) in enumerate(metas):
            recs[i] = capi.DetImage(None, 1, old_h, old_w, new_h, new_w, 0, 1.0 / (new_h / old_h), 1.0 / (new_w / old_w))
        return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(p.reg.device if dev is None else dev, non_blocking=True)


EfficientDet = EfficientDetBackbone


def _is_det_batch(inputs) -> bool:
    from .det_data import DetBatch   # det_data imports this module
    return isinstance(inputs, DetBatch)


def _check_output(output):
    if output not in ("host", "device"):
        raise ValueError(f"EfficientDet: output {output!r} (one of 'host', 'device')")
    return output


def detect_on_device(reg: torch.Tensor, cls: torch.Tensor, anchors_dev: torch.Tensor, threshold: float, iou_threshold: float,
                     records: Optional[torch.Tensor] = None):
    """detect_from_heads without the host: one launch of stlpose::det_postprocess; with `records` (the device table of
    StlDetImage records) the boxes are on the source images' scale, as invert_affine puts them.  Returns a ``Detections``."""
    from .detections import Detections
    return Detections(*torch.ops.stlpose.det_postprocess(reg, cls, anchors_dev, records, float(threshold), float(MAX_SIZE - 1),
                                                         float(MAX_SIZE - 1), float(iou_threshold)))


def detect_from_heads(reg: torch.Tensor, cls: torch.Tensor, anchors_dev: torch.Tensor, threshold: float, iou_threshold: float):
    """postprocess (efficientdet_utils/utils.py:150-187) on the device from the head outputs reg [B, A, 4] and cls [B, A, nc]:
    the decode kernel, then per image the class-aware NMS.  Returns per image (boxes float32 [k, 4] on the 512 canvas, classes
    int64 [k], scores float32 [k]) as numpy arrays, in keep order."""
    boxes, scores, classes, index, count = torch.ops.stlpose.det_decode(reg, cls, anchors_dev, float(threshold), float(MAX_SIZE - 1),
                                                                        float(MAX_SIZE - 1))
    counts = count.cpu().tolist()
    keeps = []
    for i, n in enumerate(counts):
        if n == 0:
            keeps.append(None)
            continue
        order = torch.sort(scores[i, :n], descending=True, stable=True).indices.to(torch.int32)
        keeps.append(torch.ops.stlpose.det_nms(boxes[i, :n], classes[i, :n], order, float(iou_threshold)))
    out = []
    for i, n in enumerate(counts):
        if keeps[i] is None:
            out.append((np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float32)))
            continue
        keep, kc = keeps[i]
        k = keep[:int(kc.item())].long()
        out.append((boxes[i, k].cpu().numpy(), classes[i, k].long().cpu().numpy(), scores[i, k].cpu().numpy()))
    return out


def setup_detector(model_name="faster_rcnn", model_type="", pretrained=True, num_classes=1, compute_dtype="fp32", **kwargs):
    """lib/model_setup.py:60-95.  "efficientdet" with model_type "" / "d0" or "d3" builds the reference's configuration
    (num_classes, its anchors, threshold 0.5, iou_threshold 0.5); weights come from a state_dict (load_state_dict).
    compute_dtype ("fp32", "bf16", "f16") is EfficientDetBackbone's."""
    if model_name not in ("faster_rcnn", "efficientdet"):
        raise ValueError(f"setup_detector: model_name {model_name!r} (one of 'faster_rcnn', 'efficientdet')")
    if model_type not in ("", "d0", "d3", None):
        raise ValueError(f"setup_detector: model_type {model_type!r} (one of '', 'd0', 'd3')")
    if model_name == "faster_rcnn":
        raise NotImplementedError("setup_detector: 'faster_rcnn' is torchvision's fasterrcnn_resnet50_fpn, which is not part of the "
                                  "reference's own code; use 'efficientdet'")
    cc = 3 if model_type == "d3" else 0
    return EfficientDetBackbone(compound_coef=cc, num_classes=num_classes, ratios=RATIOS, scales=SCALES, threshold=0.5,
                                iou_threshold=0.5, compute_dtype=compute_dtype)
