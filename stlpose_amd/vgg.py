"""``VGGPerceptualLoss`` on MI355X (mirror of reference ``src/lib/loss.py:17-58``).

Same call contract -- ``VGGPerceptualLoss(resize=True)(input, target) -> 0-d tensor`` on NCHW images
in [0, 1] -- and the same arithmetic: channel repeat for non-RGB, ImageNet normalisation, optional
bilinear 224x224 (align_corners=False), the four VGG16 slices ``features[0:4], [4:9], [9:16],
[16:23]`` (3x3 pad-1 convs WITH bias + ReLU, 2x2 max-pool), loss = sum over slices of mean |x - y|.

MI355X-first: input and target run as ONE batch of 2B through the implicit-GEMM conv kernel
(bias + ReLU fused in its epilogue), conv1_1's 3 input channels are fed as 3x3 patches (normalise
fused into the patch kernel) so that it is a 1x1 conv with K = 32, and each slice's L1 is a
two-level fp64 reduction.  Forward only, like the reference (its VGG is frozen and never
back-propagated through in-tree).  The trunk's weight packing (``ready``) and launch plan (``Trunk``)
serve the VGG19 losses of ``vgg19_style.py`` as well; ``pack_convs``, ``weight_table``, ``prep_weights``
and ``list_conv`` under them are every conv trunk's, AdaIN's (``adain.py``) included.

The reference takes the weights from ``torchvision.models.vgg16(pretrained=True)`` (a download);
here they come from a state_dict with the reference module's own key names
(``blocks.<slice>.<features index>.{weight,bias}``) or torchvision's (``features.<index>.*``).
Parity: fixture G10 (tests/golden/g10_vgg.npz) is the reference's own ``VGGPerceptualLoss`` run on a
torchvision-free VGG16-D layer list with synthetic weights -- its slicing, channel repeat, normalisation,
resize and L1 lines are pinned; torchvision's layer list itself (third party, absent) stays restated.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import capi
from .launch import LaunchList

# (slice, features index, cin, cout); 'p' marks a 2x2 max-pool in front of the conv
VGG16_LAYOUT = [
    (0, 0, 3, 64, False), (0, 2, 64, 64, False),
    (1, 5, 64, 128, True), (1, 7, 128, 128, False),
    (2, 10, 128, 256, True), (2, 12, 256, 256, False), (2, 14, 256, 256, False),
    (3, 17, 256, 512, True), (3, 19, 512, 512, False), (3, 21, 512, 512, False),
]
SLICE_END = {1: 0, 3: 1, 6: 2, 9: 3}  # conv position (0-based) -> slice that ends after it


def dtype_code(name: str, x3: bool = False) -> int:
    """Element type the activations are stored in.  "fp32x3" (fp32 storage, conv launches with ``math_code``'s value) is for the
    modules that say so with `x3`; the others multiply fp32 natively and refuse the name."""
    if name.lower() in ("fp32x3", "f32x3") and not x3:
        raise ValueError(f"compute_dtype {name!r} is VGGPerceptualLoss's and the pose network's; this module takes 'fp32' or 'bf16'")
    return capi.BF16 if name.lower() in ("bf16", "bfloat16") else capi.F32


def math_code(name: str) -> int:
    """``stl_conv.math`` of a compute mode: split-bf16 products for "fp32x3", the element type's own for every other."""
    return capi.MATH_BF16X3 if name.lower() in ("fp32x3", "f32x3") else capi.MATH_NATIVE


def add_conv(parent: nn.Module, idx: int, ci: int, co: int, ks: int = 3) -> nn.Module:
    """Register a frozen ks x ks conv's ``weight`` and ``bias`` as ``parent.<idx>``; returns the leaf."""
    leaf = nn.Module()
    leaf.register_parameter("weight", nn.Parameter(torch.zeros(co, ci, ks, ks), requires_grad=False))
    leaf.register_parameter("bias", nn.Parameter(torch.zeros(co), requires_grad=False))
    parent.add_module(str(idx), leaf)
    return leaf


def pack_convs(convs, dev):
    """[(weight, bias)] in launch order -> (``w_flat``, ``bias_flat``: fp32 on `dev`; ``bias_off``: each conv's first bias)."""
    bias_off, off = [], 0
    for _, b in convs:
        bias_off.append(off)
        off += b.numel()
    w_flat = torch.cat([w.detach().reshape(-1).float() for w, _ in convs]).to(dev).contiguous()
    return w_flat, torch.cat([b.detach().float() for _, b in convs]).to(dev).contiguous(), bias_off


def ready(mod: nn.Module, dev) -> None:
    """Move a VGG loss to `dev` and pack the convs of ``mod._convs`` there in layout order (``pack_convs``).  A repack drops
    ``mod._plans``: their launches point into the old buffers."""
    if mod.mean.device != dev:
        mod.to(dev)
    if mod._flat_dev != dev:
        mod.w_flat, mod.bias_flat, mod.bias_off = pack_convs([(leaf.weight, leaf.bias) for leaf in mod._convs], dev)
        mod._flat_dev = dev
        mod._plans.clear()


def weight_table(rows, grad: bool = False):
    """The ``capi.WPrep`` table of the 3x3 convs ``rows`` = [(cin, cout)] packed by ``pack_convs`` -> (table, elements of the
    kernel-layout buffer ``wk``, blocks of stl_weight_prep).  The first conv is a 1x1 conv on 32-wide 3x3 patches ([Co][32],
    data gradient [32][Co]).  grad: ``wk`` also holds the data-gradient layouts [Ci][flipped tap][Co] (``bwd_off``): the
    forward layouts' sizes, in the same order, behind them."""
    tab = (capi.WPrep * len(rows))()
    src = off = blk = 0
    for i, (ci, co) in enumerate(rows):
        patch = i == 0
        cip, kk = (32, 1) if patch else (ci, 9)
        e = tab[i]
        e.src_off, e.fwd_off, e.bwd_off = src, off, -1
        e.Co, e.Ci, e.ks, e.Cip, e.patch, e.blk0 = co, ci, 3, cip, int(patch), blk
        src += co * ci * 9
        off += co * kk * cip
        blk += math.ceil(co * ci * 9 / 1024)
    if grad:
        for e in tab:
            e.bwd_off = off + e.fwd_off
        off *= 2
    return tab, off, blk


def prep_weights(dt: int, w_flat, wk, wtab_dev, n: int, blocks: int, stream: int) -> None:
    """``w_flat`` -> the kernel layouts of the table's `n` convs in ``wk``."""
    capi.call("stl_weight_prep", dt, w_flat.data_ptr(), wk.data_ptr(), wtab_dev.data_ptr(), n, blocks, stream)


def list_conv(ops: LaunchList, dt: int, B, h, w, ci, co, ks, src, wptr, out, bias=0, out_relu=0, addend=0, mask_z=0, math=0) -> None:
    """List a stride-1 'same' conv of the NHWC map at `src` onto `out` in `ops`."""
    p = capi.Conv()
    p.math = math
    p.dtype, p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co = dt, B, h, w, ci, h, w, co
    p.ks, p.stride, p.shape = ks, 1, -1
    p.src.x, p.src.mode = src, capi.SRC_PLAIN
    p.w, p.out, p.bias, p.out_relu, p.addend, p.mask_z = wptr, out, bias, out_relu, addend, mask_z
    capi.call("stl_conv_plan", C.byref(p))
    ops.add("stl_conv_forward", p)


class Trunk:
    """Static launch list of a VGG trunk for one batch geometry: nb images of H x W through the 3x3 convs
    ``rows`` = [(cin, cout, 2x2 max-pool in front)] of a module packed by ``ready``, each with bias + ReLU.

    ``hook(trunk, i)`` runs right after conv i is listed and may list launches of its own behind it.  grad: ``wk`` also
    holds the data-gradient layouts of the convs behind the forward ones (``tab[i].bwd_off``).  ``ops`` is the forward
    ``LaunchList``; the plan holds every buffer its launches point into (``keep``, the list's)."""

    def __init__(self, mod: nn.Module, rows, nb: int, H: int, W: int, dev, hook, grad: bool = False):
        self.ops = LaunchList()
        self.keep, self.acts, self.dims = self.ops.keep, [], []   # acts, dims: per conv its output [nb, h, w, co], (h, w, co)
        self.dt = mod.dtype
        self.math = getattr(mod, "math", capi.MATH_NATIVE)   # VGGPerceptualLoss(compute_dtype="fp32x3"): on every conv launch
        self.esz, self.tdt = capi.DTYPES[self.dt]
        self.w_flat = mod.w_flat
        self.img = torch.zeros(nb, 3, H, W, device=dev)
        self.tab, wk_elems, self.wblocks = weight_table([row[:2] for row in rows], grad)
        self.wk = torch.zeros(wk_elems, dtype=self.tdt, device=dev)
        self.wtab = torch.frombuffer(bytearray(bytes(self.tab)), dtype=torch.uint8).clone().to(dev)

        def act(b, h, w, c):
            t = torch.empty(b * h * w * c * self.esz, dtype=torch.uint8, device=dev)
            self.keep.append(t)
            return t

        x = act(nb, H, W, 32)
        self.ops.add("stl_patch3x3", self.dt, self.img.data_ptr(), x.data_ptr(), nb, H, W, 1, mod.mean.data_ptr(), mod.std.data_ptr())
        h, w, c = H, W, 32
        for i, (_, co, pool) in enumerate(rows):
            if pool:
                y = act(nb, h // 2, w // 2, c)
                self.ops.add("stl_maxpool2x2", self.dt, x.data_ptr(), y.data_ptr(), nb, h, w, c)
                x, h, w = y, h // 2, w // 2
            y = act(nb, h, w, co)
            list_conv(self.ops, self.dt, nb, h, w, c, co, 1 if i == 0 else 3, x.data_ptr(), self.wk.data_ptr() + self.tab[i].fwd_off * self.esz,
                      y.data_ptr(), bias=mod.bias_flat.data_ptr() + 4 * mod.bias_off[i], out_relu=1, math=self.math)
            x, c = y, co
            self.acts.append(y)
            self.dims.append((h, w, c))
            hook(self, i)

    def prep_weights(self, st) -> None:
        """``w_flat`` -> the kernel layouts in ``wk``."""
        prep_weights(self.dt, self.w_flat, self.wk, self.wtab, len(self.tab), self.wblocks, st)


class VGGPerceptualLoss(nn.Module):
    def __init__(self, resize: bool = True, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 compute_dtype: str = "fp32"):
        super().__init__()
        self.resize = resize
        self.dtype, self.math = dtype_code(compute_dtype, x3=True), math_code(compute_dtype)
        self.blocks = nn.ModuleList([nn.Module() for _ in range(4)])  # reference: self.blocks[s][features idx]
        self._convs = [add_conv(self.blocks[s], idx, ci, co) for s, idx, ci, co, _ in VGG16_LAYOUT]
        self.mean = nn.Parameter(torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))   # loss.py:37
        self.std = nn.Parameter(torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))    # loss.py:38
        self._plans: Dict = {}
        self._flat_dev = None
        if state_dict is not None:
            self.load_vgg_weights(state_dict)

    def load_vgg_weights(self, sd: Dict[str, torch.Tensor]):
        """Accepts torchvision's ``features.<idx>.*`` keys or the reference module's ``blocks.<s>.<idx>.*``."""
        with torch.no_grad():
            for (s, idx, _, _, _), leaf in zip(VGG16_LAYOUT, self._convs):
                for name in ("weight", "bias"):
                    t = sd.get(f"features.{idx}.{name}", sd.get(f"blocks.{s}.{idx}.{name}"))
                    if t is None:
                        raise KeyError(f"VGG16 weights: missing features.{idx}.{name}")
                    getattr(leaf, name).copy_(t)
        self._flat_dev = None

    def _plan(self, B2: int, H: int, W: int, dev):
        """(trunk plan for one (2B, H, W) shape with each slice's L1 term behind its last conv, the loss it sums into)."""
        partial = torch.zeros(4, 1024, dtype=torch.float64, device=dev)
        loss = torch.zeros((), dtype=torch.float32, device=dev)

        def l1(t, i):
            if i in SLICE_END:
                s, x = SLICE_END[i], t.acts[i].data_ptr()
                h, w, c = t.dims[i]
                half = (B2 // 2) * h * w * c
                t.ops.add("stl_l1_partial", t.dt, x, x + half * t.esz, half, partial[s].data_ptr(), 1024)
                t.ops.add("stl_sum_partials", partial[s].data_ptr(), 1024, 1.0 / half, loss.data_ptr(), int(s > 0))

        trunk = Trunk(self, [row[2:] for row in VGG16_LAYOUT], B2, H, W, dev, l1)
        trunk.ops.keep_alive(partial)
        return trunk, loss

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not input.is_cuda:
            raise RuntimeError("stlpose_amd.VGGPerceptualLoss runs only on an MI355X (cuda/HIP device); there is no CPU path")
        if input.shape[1] != 3:  # loss.py:43-45
            input, target = input.repeat(1, 3, 1, 1), target.repeat(1, 3, 1, 1)
        dev = input.device
        ready(self, dev)
        st = torch.cuda.current_stream().cuda_stream
        x = torch.cat([input, target.to(dev)], 0).contiguous().float()
        B2, _, H, W = x.shape
        if self.resize:  # bilinear commutes with the per-channel affine normalisation (weights sum to 1)
            r = torch.empty(B2, 3, 224, 224, device=dev)
            capi.call("stl_bilinear_nchw", x.data_ptr(), r.data_ptr(), B2, 3, H, W, 224, 224, st)
            x, H, W = r, 224, 224
        if H < 8 or W < 8:   # three 2x2 max-pools (floor, like nn.MaxPool2d) must leave at least one pixel
            raise RuntimeError(f"VGGPerceptualLoss needs H, W >= 8, got {H}x{W}")
        key = (B2, H, W)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._plan(B2, H, W, dev)
        trunk, loss = plan
        trunk.img.copy_(x)
        trunk.prep_weights(st)
        trunk.ops.run(st)
        return loss.clone()
