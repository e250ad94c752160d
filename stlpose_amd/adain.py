"""AdaIN feed-forward stylisation on MI355X (Huang & Belongie 2017): one encoder pass, one per-channel affine and one decoder
pass per image -- the step that makes Styled-COCO (``images_style_{styles}_alpha_{alpha}``, reference
``src/data/data_loaders.py:83-100``) out of COCO and a set of style images.

No reference counterpart: the reference only READS the stylised images, the code that makes them is not in its tree (as with
``VGG19StyleLoss``).  PARITY UNPINNED by construction; the yardstick is ``tests/adain_ref.py``, a plain
PyTorch restatement of the published network.  No weight file is at hand either: the key layout of the published files
(``vgg_normalised.pth``, ``decoder.pth``) and the arithmetic are pinned, the published checkpoints' outputs are not.

Network (the published layout, so that the published weight files load).  Encoder: the "normalised VGG19" up to relu4_1, an
``nn.Sequential`` of 31 entries -- a 1x1 conv 3->3 at index 0, then ReflectionPad2d(1) + 3x3 conv + ReLU groups with the convs
at ``ENCODER_LAYOUT``'s indices and ``MaxPool2d(2, 2, ceil_mode=True)`` at 7, 14, 27.  Decoder: 29 entries, reflection pad +
3x3 conv (+ ReLU except after the last) at ``DECODER_LAYOUT``'s indices and nearest x2 upsampling at 3, 16, 23.  AdaIN on the
relu4_1 features, per image and channel over the pixels: ``t = s_s * (f - m_c) / s_c + m_s`` with ``s = sqrt(var_unbiased + 1e-5)``,
then ``t <- alpha * t + (1 - alpha) * f``: together ONE affine per (image, channel), ``affine_coefficients``.

MI355X-first.  The 3x3 convs run on the implicit-GEMM ``stl_conv_forward`` (bias + ReLU in its epilogue) exactly as
``vgg.list_conv`` lists them.  That kernel pads with zeros, so each layer is: ``stl_reflect_gather`` writes the explicitly
reflection-padded (H+2) x (W+2) NHWC map -- with the max-pool / upsample that sits between two convs, and in front of the
decoder the AdaIN affine, fused in -- the conv runs as a "same" conv on it, and the next gather reads only the interior of that
output (DESIGN.md "AdaIN: the ring").  The 1x1 conv at encoder index 0 is folded into conv1_1 on the host (exact: the padding
behind it is a reflection, every tap sees a real pixel), and conv1_1 is a 1x1 conv on 32-wide reflection patches
(``stl_adain_input``).  The transformed features are never written on their own.  Inference only.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import capi
from .launch import LaunchList
from .vgg import add_conv, dtype_code, list_conv, pack_convs, prep_weights, weight_table

# (Sequential index, cin, cout, op in front of the conv's reflection pad: None, "pool" or "up")
ENCODER_LAYOUT = [(2, 3, 64, None), (5, 64, 64, None), (9, 64, 128, "pool"), (12, 128, 128, None), (16, 128, 256, "pool"),
                  (19, 256, 256, None), (22, 256, 256, None), (25, 256, 256, None), (29, 256, 512, "pool")]
DECODER_LAYOUT = [(1, 512, 256, None), (5, 256, 256, "up"), (8, 256, 256, None), (11, 256, 256, None), (14, 256, 128, None),
                  (18, 128, 128, "up"), (21, 128, 64, None), (25, 64, 64, "up"), (28, 64, 3, None)]
EPS = 1e-5
FEAT = 512        # channels of relu4_1
OUT_CO = 8        # the last conv's 3 output channels, zero-padded to stl_conv's minimum
_OPS = {None: capi.GATHER_COPY, "up": capi.GATHER_UP, "pool": capi.GATHER_POOL}

StyleStats = Tuple[torch.Tensor, torch.Tensor]


def fold_input_conv(w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor):
    """The 1x1 conv (w0 [3,3,1,1], b0) followed by reflection pad + conv1_1 (w1 [64,3,3,3], b1) as ONE reflection-padded 3x3 conv:
    ``W'[o,i,ky,kx] = sum_m W1[o,m,ky,kx] W0[m,i]``, ``b'[o] = b1[o] + sum_{m,ky,kx} W1[o,m,ky,kx] b0[m]``.  Exact because the
    padding is a reflection: every tap sees a real pixel, so the inner bias reaches every tap."""
    w0 = w0.reshape(w0.shape[0], w0.shape[1]).double()
    w = torch.einsum("omyx,mi->oiyx", w1.double(), w0)
    b = b1.double() + torch.einsum("omyx,m->o", w1.double(), b0.double())
    return w.to(w1.dtype), b.to(b1.dtype)


def affine_coefficients(mean_c: torch.Tensor, var_c: torch.Tensor, mean_s: torch.Tensor, sigma_s: torch.Tensor, alpha: float,
                        style_weights: Optional[torch.Tensor] = None, eps: float = EPS):
    """(scale, offset) [B, C] with ``alpha * adain(f) + (1 - alpha) * f == f * scale + offset``: the host statement of
    ``stl_adain_affine``.  mean_c, var_c [B, C] (unbiased variance of the content features); mean_s, sigma_s [S, C] with
    sigma = sqrt(var + eps); S = 1 (one style for the batch), S = B (one per image), or any S with style_weights [B, S] whose rows
    sum to 1: ``s_s = sum_k w_k s_k``, ``m_s = sum_k w_k m_k`` (the published interpolation)."""
    B, S = mean_c.shape[0], mean_s.shape[0]
    w = mix_matrix(B, S, style_weights).to(mean_s.dtype)
    ms, ss = w @ mean_s, w @ sigma_s
    r = ss / torch.sqrt(var_c + eps)
    return alpha * r + (1.0 - alpha), alpha * (ms - mean_c * r)


def mix_matrix(B: int, S: int, style_weights: Optional[torch.Tensor]) -> torch.Tensor:
    """[B, S] weights of the S prepared styles for each of the B images (in the dtype given; fp32 for the built-in cases)."""
    if style_weights is not None:
        w = torch.as_tensor(style_weights)
        w = w if w.is_floating_point() else w.float()
        if tuple(w.shape) != (B, S):
            raise ValueError(f"style_weights must be [{B}, {S}] (images x styles), got {tuple(w.shape)}")
        if not torch.allclose(w.sum(1), torch.ones(B, dtype=w.dtype), atol=1e-4):
            raise ValueError("style_weights: every row must sum to 1")
        return w
    if S == 1:
        return torch.ones(B, 1)
    if S == B:
        return torch.eye(B)
    raise ValueError(f"{S} styles for {B} content images: pass 1 style, {B} styles, or style_weights [{B}, {S}]")


def check_size(what: str, H: int, W: int) -> None:
    if H % 8 or W % 8 or H < 16 or W < 16:
        raise ValueError(f"AdaINStylizer: {what} size {H}x{W}: H and W must be multiples of 8 and at least 16 (ceil-mode pooling "
                         "then equals floor pooling, and the reflection at relu4_1 has the 2 pixels it needs)")


class _Plan:
    """Static launch list for nb images of H x W: the encoder up to relu4_1 with its statistics and, with ``decode``, the
    decoder behind the affine gather.  Two buffers alternate: a gather writes ``pad``, the conv reads it and writes ``act``,
    the next gather reads ``act``.  Holds every buffer the launches of ``encode`` and ``decode`` (LaunchLists, one ``keep``) point into."""

    def __init__(self, mod: "AdaINStylizer", nb: int, H: int, W: int, dev, decode: bool):
        self.dt, self.esz = mod.dtype, capi.DTYPES[mod.dtype][0]
        self.nb, self.H, self.W = nb, H, W
        self.img = torch.zeros(nb, 3, H, W, device=dev)
        dt, nb_ = self.dt, nb
        # sizes first: the largest padded input and the largest conv output
        layers, h, w = [], H, W
        for li, (_, ci, co, op) in enumerate(ENCODER_LAYOUT + (DECODER_LAYOUT if decode else [])):
            if op == "pool":
                h, w = h // 2, w // 2
            elif op == "up":
                h, w = 2 * h, 2 * w
            layers.append((li, ci, co, op, h, w))
        pad_n = max(nb * (h + 2) * (w + 2) * ci for li, ci, co, op, h, w in layers if li > 0)
        act_n = max(nb * H * W * 64, max(nb * (h + 2) * (w + 2) * max(co, OUT_CO) for li, ci, co, op, h, w in layers if li > 0))
        self.patch = torch.empty(nb * H * W * 32 * self.esz, dtype=torch.uint8, device=dev)
        self.pad = torch.empty(pad_n * self.esz, dtype=torch.uint8, device=dev)
        self.act = torch.empty(act_n * self.esz, dtype=torch.uint8, device=dev)
        h8, w8 = H // 8, W // 8
        self.nchunk = max(1, min(64, math.ceil(1024 / nb), (h8 * w8) // 8))
        self.partial = torch.empty(nb * self.nchunk * 2 * FEAT, dtype=torch.float64, device=dev)
        self.mean, self.var, self.sigma = (torch.empty(nb, FEAT, device=dev) for _ in range(3))
        self.scale, self.offset = torch.empty(nb, FEAT, device=dev), torch.empty(nb, FEAT, device=dev)
        self.out = torch.empty(nb, 3, H, W, device=dev)
        pad, act = self.pad.data_ptr(), self.act.data_ptr()

        def conv(ops, li, h, w, ci, co, ks, src, relu):
            list_conv(ops, dt, nb_, h, w, ci, co, ks, src, mod.wk.data_ptr() + mod.wtab[li].fwd_off * self.esz, act,
                      bias=mod.bias_flat.data_ptr() + 4 * mod.bias_off[li], out_relu=relu)

        # ---- encoder: conv1_1 (with the 1x1 input conv folded in) on reflection patches, then gather -> conv per layer
        self.encode = ops = LaunchList()
        ops.add("stl_adain_input", dt, self.img.data_ptr(), self.patch.data_ptr(), nb, H, W)
        conv(ops, 0, H, W, 32, 64, 1, self.patch.data_ptr(), 1)
        ph, pw, ring = H, W, 0          # interior size and ring of what `act` holds
        for li, ci, co, op, h, w in layers[1:len(ENCODER_LAYOUT)]:
            ops.add("stl_reflect_gather", dt, act, pad, nb, ph, pw, ring, ci, _OPS[op], 0, 0)
            conv(ops, li, h + 2, w + 2, ci, co, 3, pad, 1)
            ph, pw, ring = h, w, 1
        ops.add("stl_adain_stats", dt, act, nb, h8, w8, 1, FEAT, self.nchunk, self.partial.data_ptr(), EPS, self.mean.data_ptr(),
                self.var.data_ptr(), self.sigma.data_ptr())
        # ---- decoder: the affine rides on the first gather; stl_adain_output is launched by stylise() (`clamp` is its argument)
        self.decode = ops = LaunchList(self.encode.keep)
        if decode:
            for li, ci, co, op, h, w in layers[len(ENCODER_LAYOUT):]:
                first = li == len(ENCODER_LAYOUT)
                ops.add("stl_reflect_gather", dt, act, pad, nb, ph, pw, ring, ci, _OPS[op],
                        self.scale.data_ptr() if first else 0, self.offset.data_ptr() if first else 0)
                last = li == len(layers) - 1
                conv(ops, li, h + 2, w + 2, ci, OUT_CO if last else co, 3, pad, 0 if last else 1)
                ph, pw = h, w


class AdaINStylizer(nn.Module):
    """``AdaINStylizer(encoder_sd, decoder_sd).stylise(content, style, alpha)`` -> stylised NCHW fp32 images.

    Parameters live as ``encoder.<idx>.{weight,bias}`` / ``decoder.<idx>.{weight,bias}`` (frozen, unfolded), so ``state_dict()``
    holds both published files' keys under two prefixes."""

    def __init__(self, encoder_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 decoder_state_dict: Optional[Dict[str, torch.Tensor]] = None, compute_dtype: str = "fp32"):
        super().__init__()
        if compute_dtype.lower() not in ("fp32", "float32", "bf16", "bfloat16"):
            raise ValueError(f"compute_dtype must be 'fp32' or 'bf16', got {compute_dtype!r}")
        self.dtype = dtype_code(compute_dtype)
        self.encoder, self.decoder = nn.Module(), nn.Module()
        add_conv(self.encoder, 0, 3, 3, 1)
        for idx, ci, co, _ in ENCODER_LAYOUT:
            add_conv(self.encoder, idx, ci, co)
        for idx, ci, co, _ in DECODER_LAYOUT:
            add_conv(self.decoder, idx, ci, co)
        self._plans: Dict = {}
        self._flat_dev = None
        if encoder_state_dict is not None:
            self.load_encoder_weights(encoder_state_dict)
        if decoder_state_dict is not None:
            self.load_decoder_weights(decoder_state_dict)

    # ---------------------------------------------------------------- weights
    def _load(self, part: nn.Module, what: str, idxs, sd) -> None:
        with torch.no_grad():
            for idx in idxs:
                for name in ("weight", "bias"):
                    key = f"{idx}.{name}"
                    if key not in sd:
                        raise KeyError(f"AdaIN {what} weights: missing key '{key}'")
                    getattr(getattr(part, str(idx)), name).copy_(sd[key])
        self._flat_dev = None

    def load_encoder_weights(self, sd: Dict[str, torch.Tensor]) -> None:
        """Keys ``0.weight, 0.bias, 2.weight, ... 29.bias`` as in ``vgg_normalised.pth``; a file of the whole VGG19 (conv indices
        above 29) loads, the rest is ignored."""
        self._load(self.encoder, "encoder", [0] + [r[0] for r in ENCODER_LAYOUT], sd)

    def load_decoder_weights(self, sd: Dict[str, torch.Tensor]) -> None:
        """Keys ``1.weight, ... 28.bias`` as in ``decoder.pth``."""
        self._load(self.decoder, "decoder", [r[0] for r in DECODER_LAYOUT], sd)

    def folded_conv1_1(self):
        """(weight [64,3,3,3], bias [64]) of encoder.0 folded into encoder.2."""
        e0, e2 = getattr(self.encoder, "0"), getattr(self.encoder, "2")
        return fold_input_conv(e0.weight.detach(), e0.bias.detach(), e2.weight.detach(), e2.bias.detach())

    def _pack(self, dev) -> None:
        """The host half of ``_ready``: the 18 convs in launch order on `dev` (``vgg.pack_convs``: conv1_1 folded, the last conv's
        Co zero-padded to the conv's minimum), their weight table and the still empty kernel-layout buffer ``wk``.  Drops the
        plans: their launches point into the old buffers."""
        self.to(dev)
        convs = [self.folded_conv1_1()]
        for part, layout in ((self.encoder, ENCODER_LAYOUT[1:]), (self.decoder, DECODER_LAYOUT)):
            for idx, _, _, _ in layout:
                leaf = getattr(part, str(idx))
                convs.append((leaf.weight.detach(), leaf.bias.detach()))
        w, b = convs[-1]   # 64 -> 3
        convs[-1] = (torch.cat([w, w.new_zeros(OUT_CO - 3, *w.shape[1:])]), torch.cat([b, b.new_zeros(OUT_CO - 3)]))
        self.w_flat, self.bias_flat, self.bias_off = pack_convs(convs, dev)
        self.wtab, wk_elems, self.wblocks = weight_table([(w.shape[1], w.shape[0]) for w, _ in convs])
        self.wk = torch.zeros(wk_elems, dtype=capi.DTYPES[self.dtype][1], device=dev)
        self._wtab_dev = torch.frombuffer(bytearray(bytes(self.wtab)), dtype=torch.uint8).clone().to(dev)
        self._plans.clear()

    def _ready(self, dev) -> None:
        """Pack the convs on `dev` and lay them out for the conv kernel, once per (re)pack: the weights are frozen."""
        if self._flat_dev != dev:
            self._pack(dev)
            prep_weights(self.dtype, self.w_flat, self.wk, self._wtab_dev, len(self.wtab), self.wblocks,
                         torch.cuda.current_stream().cuda_stream)
            self._flat_dev = dev

    # ---------------------------------------------------------------- checks shared by the entry points
    @staticmethod
    def _images(what: str, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"AdaINStylizer: {what} must be a [B, 3, H, W] tensor, got {tuple(getattr(x, 'shape', ()))}")
        check_size(what, x.shape[2], x.shape[3])
        if not x.is_cuda:
            raise RuntimeError("stlpose_amd.AdaINStylizer runs only on an MI355X (cuda/HIP device); there is no CPU path")
        if x.requires_grad:
            raise NotImplementedError("AdaINStylizer is inference only: an input that requires grad has no backward here")
        return x.detach().float().contiguous()

    def _plan(self, dev, nb: int, H: int, W: int, decode: bool) -> _Plan:
        key = (nb, H, W, self.dtype, decode)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _Plan(self, nb, H, W, dev, decode)
        return plan

    # ---------------------------------------------------------------- public
    @torch.no_grad()
    def prepare_style(self, style: torch.Tensor) -> StyleStats:
        """(mean, sigma) [S, 512] fp32 of the relu4_1 features of S style images: what ``stylise`` needs of a style."""
        style = self._images("style", style)
        dev = style.device
        self._ready(dev)
        S, _, h, w = style.shape
        plan = self._plan(dev, S, h, w, False)
        plan.img.copy_(style)
        plan.encode.run(torch.cuda.current_stream().cuda_stream)
        return plan.mean.clone(), plan.sigma.clone()

    @torch.no_grad()
    def stylise(self, content: torch.Tensor, style: Union[torch.Tensor, StyleStats], alpha: float = 1.0, clamp: bool = True,
                style_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """content [B,3,H,W] in [0,1] on the GPU -> [B,3,H,W] fp32.  style: [1,3,h,w] (one for the batch), [B,3,h,w] (one per
        image), any [S,3,h,w] with style_weights [B,S], or the (mean, sigma) of ``prepare_style``; its size is independent of
        the content's.  H, W, h, w: multiples of 8, at least 16."""
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"AdaINStylizer: alpha must lie in [0, 1], got {alpha}")
        content = self._images("content", content)
        dev = content.device
        if isinstance(style, (tuple, list)):
            mean_s, sigma_s = (t.to(dev, torch.float32).contiguous() for t in style)
            if mean_s.dim() != 2 or mean_s.shape[1] != FEAT or mean_s.shape != sigma_s.shape:
                raise ValueError(f"AdaINStylizer: prepared style must be (mean, sigma) of shape [S, {FEAT}]")
        else:
            mean_s, sigma_s = self.prepare_style(style)
        B, _, H, W = content.shape
        S = mean_s.shape[0]
        wmix = mix_matrix(B, S, None if style_weights is None else torch.as_tensor(style_weights).detach().cpu()).to(dev, torch.float32).contiguous()
        self._ready(dev)
        st = torch.cuda.current_stream().cuda_stream
        plan = self._plan(dev, B, H, W, True)
        plan.img.copy_(content)
        plan.encode.run(st)
        capi.call("stl_adain_affine", plan.mean.data_ptr(), plan.var.data_ptr(), mean_s.data_ptr(), sigma_s.data_ptr(), wmix.data_ptr(),
                  B, FEAT, S, float(alpha), EPS, plan.scale.data_ptr(), plan.offset.data_ptr(), st)
        plan.decode.run(st)
        capi.call("stl_adain_output", self.dtype, plan.act.data_ptr(), plan.out.data_ptr(), B, H, W, OUT_CO, int(bool(clamp)), st)
        return plan.out.clone()

    forward = stylise


def conv_macs(B: int, H: int, W: int, padded: bool, decode: bool = True) -> int:
    """Multiply-accumulates of the 9 (+ 9) convs for B images of H x W: at the (h+2) x (w+2) maps the kernels run on
    (padded) or at the network's true h x w maps.  conv1_1 counts its 27 real taps (it runs on patches, without a ring)."""
    total, h, w = 0, H, W
    for li, (_, ci, co, op) in enumerate(ENCODER_LAYOUT + (DECODER_LAYOUT if decode else [])):
        if op == "pool":
            h, w = h // 2, w // 2
        elif op == "up":
            h, w = 2 * h, 2 * w
        px = (h + 2) * (w + 2) if (padded and li > 0) else h * w
        total += B * px * ci * co * 9
    return total


def stream_bytes(B: int, H: int, W: int, esz: int, decode: bool = True) -> Dict[str, int]:
    """Bytes the streaming kernels must move for B images of H x W (each source vector read once, each output written once)."""
    gather, h, w = 0, H, W
    for li, (_, ci, co, op) in enumerate(ENCODER_LAYOUT + (DECODER_LAYOUT if decode else [])):
        ph, pw = h, w
        if op == "pool":
            h, w = h // 2, w // 2
        elif op == "up":
            h, w = 2 * h, 2 * w
        if li > 0:
            gather += B * ci * esz * (ph * pw + (h + 2) * (w + 2))
    return {"input": B * H * W * (3 * 4 + 32 * esz), "gather": gather, "stats": B * (H // 8) * (W // 8) * FEAT * esz,
            "output": (B * H * W * (OUT_CO * esz + 3 * 4)) if decode else 0}
