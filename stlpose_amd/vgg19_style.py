"""VGG19 perceptual style-transfer loss on MI355X: content (relu4_2 MSE) + Gram-matrix style loss
(relu1_1 .. relu5_1) -- the forward pass BASELINE.json configs[3] names ("VGG19 perceptual style-transfer forward
(content + Gram style loss) 512x512 bs=16 fp32").

**No reference counterpart** (SURVEY.md 8a, row V2): /root/reference contains only the VGG16 + L1
``VGGPerceptualLoss`` (``lib/loss.py:17-58`` -> ``stlpose_amd/vgg.py``); this module follows the published method
(Gatys et al. 2016, Johnson et al. 2016) and is checked against ``oracle.vgg_ref.vgg19_style_content_loss`` only:
PARITY UNPINNED.

MI355X-first, on the same kernels as the V1 path: the stylised / content / style images run as ONE batch of 3B
through the implicit-GEMM conv kernel (bias + ReLU in its epilogue; conv1_1 as 27 -> 32-wide patches with the
ImageNet normalisation fused into the patch kernel), 2x2 max-pools, and every Gram matrix G = F F^T / (C H W) is
the MFMA weight-gradient kernel run as a 1x1 "convolution" of the NHWC feature map with itself
(dw[c1][c2] = sum_pixels F[p][c1] F[p][c2]: K = pixels, transposed LDS reads, split-K slabs), one launch per image
and tap.  The content term is a two-level fp64 reduction of squared differences (``stl_l2_partial``).

Differentiable in the stylised images: with ``x.requires_grad`` the plan (keyed by a grad flag; without it the plan and its launches
are exactly the forward ones) also holds the image gradient of images [0, B) -- 13 data gradients on the transposed weights with
the ReLU masks in their epilogue (``mask_z``), the max-pool adjoints (``stl_maxpool2x2_backward``), per image and style tap a 1x1
conv with weight 4 / (B C^3 HW) * (G_b - A_b) whose epilogue adds the gradient from deeper layers, the content term
(``stl_l2_backward``) and the patch adjoint (``stl_patch3x3_backward``) to the NCHW image.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import capi
from .launch import LaunchList
from .vgg import Trunk, add_conv, dtype_code, list_conv, ready

# (features index, cin, cout, 2x2 max-pool in front): torchvision VGG19 "E" up to conv5_1
VGG19_LAYOUT = [(0, 3, 64, False), (2, 64, 64, False), (5, 64, 128, True), (7, 128, 128, False), (10, 128, 256, True),
                (12, 256, 256, False), (14, 256, 256, False), (16, 256, 256, False), (19, 256, 512, True), (21, 512, 512, False),
                (23, 512, 512, False), (25, 512, 512, False), (28, 512, 512, True)]
STYLE_TAPS = (0, 2, 4, 8, 12)   # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1
CONTENT_TAP = 9                 # relu4_2


def vgg19_flops_per_image(H: int, W: int) -> float:
    """2 * MACs of the 13 convolutions up to conv5_1."""
    fl, h, w = 0.0, H, W
    for _, ci, co, pool in VGG19_LAYOUT:
        if pool:
            h, w = h // 2, w // 2
        fl += 2.0 * h * w * co * ci * 9
    return fl


class StylePlan:
    """The native launches of one batch geometry: the VGG19 trunk (``self.trunk``) with the content and Gram terms at their taps.

    nb images of H x W run as one batch.  content = "batch": the content term compares images [0, B) with [B, 2B) of the batch
    (VGG19StyleLoss: stylised, content, style); "buffer": with the relu4_2 features in ``self.ctarget`` (the stylisation driver's
    cached targets); None: no content term.  gram_imgs: the images whose Gram matrices are formed, in slab order.
    grad: also plan the image gradient of images [0, B) (``self.bwd_ops``); a plan without it is exactly the forward plan."""

    def __init__(self, mod: "VGG19StyleLoss", nb: int, H: int, W: int, dev, B: int, content: Optional[str], gram_imgs,
                 grad: bool = False):
        self.B, self.H, self.W = B, H, W
        self.cpartial = torch.zeros(1024, dtype=torch.float64, device=dev)
        self.content = torch.zeros((), dtype=torch.float32, device=dev)
        self.slabs = []   # per style tap: (slabs [len(gram_imgs), nsplit, C, C] fp32, 1 / (C H W))

        def taps(t, i):
            dt, esz = t.dt, t.esz
            h, w, c = t.dims[i]
            x = t.acts[i].data_ptr()
            img_elems = h * w * c
            if i == CONTENT_TAP and content is not None:   # images [0, B) = stylised; target: images [B, 2B) or the cached buffer
                n = B * img_elems
                if content == "batch":
                    tgt = x + n * esz
                else:
                    self.ctarget = torch.zeros(n, dtype=t.tdt, device=dev)
                    tgt = self.ctarget.data_ptr()
                t.ops.add("stl_l2_partial", dt, x, tgt, n, self.cpartial.data_ptr(), 1024)
                t.ops.add("stl_sum_partials", self.cpartial.data_ptr(), 1024, 1.0 / n, self.content.data_ptr(), 0)
                self.ctarget_ptr = tgt
            if i in STYLE_TAPS and len(gram_imgs):
                from .engine import choose_tile
                th, tw = choose_tile(1, h, w, 1, 1, esz, bn_cols=32, maxhalo=576)
                npt = math.ceil((h + 1) / th) * math.ceil(w / tw)
                shape = (dt, 1, h, w, c, h, w, c, 1, 1)   # one image's map as a 1x1 conv of itself: dtype, B, Hi, Wi, Ci, Ho, Wo, Co, ks, stride
                ctile = capi.lib().stl_wgrad_chunk(C.byref(capi.Wgrad(*shape)))
                chunks = math.ceil(c / ctile) ** 2
                nsplit = max(1, min(npt, max(1, 256 // chunks)))
                slabs = torch.zeros(len(gram_imgs), nsplit, c, c, dtype=torch.float32, device=dev)
                for j, b in enumerate(gram_imgs):
                    wg = capi.Wgrad(*shape, th, tw, nsplit)
                    ptr = x + b * img_elems * esz
                    wg.h.x, wg.h.mode, wg.g.x, wg.g.mode = ptr, capi.SRC_PLAIN, ptr, capi.SRC_PLAIN
                    wg.partial = slabs[j].data_ptr()
                    t.ops.add("stl_conv_wgrad", wg)
                self.slabs.append((slabs, 1.0 / (c * h * w)))

        self.trunk = Trunk(mod, [row[1:] for row in VGG19_LAYOUT], nb, H, W, dev, taps, grad)
        if grad:
            self._plan_backward(mod, dev)

    def grams(self) -> List[torch.Tensor]:
        """Per style tap the Gram matrices [len(gram_imgs), C, C] fp64 of the last forward run: its split-K slabs summed."""
        return [slabs.double().sum(1) * scale for slabs, scale in self.slabs]

    def _plan_backward(self, mod, dev) -> None:
        """Image gradient of images [0, B): the 13 data gradients (stl_conv_forward on the transposed weights, ReLU masks from
        the stored outputs as mask_z), the max-pool adjoints, the Gram terms (a 1x1 conv per image and tap with the weight
        ks * (G_b - A_b), the gradient from deeper layers as addend), the content term (stl_l2_backward, in place) and the patch
        adjoint.  Gradients ping-pong between two buffers per resolution."""
        t, B = self.trunk, self.B
        dt, esz = t.dt, t.esz
        self.bwd_ops = LaunchList(t.keep)   # shares the trunk's keep
        self.cscale = torch.zeros((), dtype=torch.float32, device=dev)   # 2 wc / n, set by backward()
        self.gw = {}                                                     # style tap -> [B, C, C] weight ks * (G_b - A_b)
        self.dimg = torch.zeros(B, 3, self.H, self.W, dtype=torch.float32, device=dev)
        bufs = self.gbufs = {}   # (h, w) -> two buffers; held by the plan: the ops keep raw pointers into them

        def other(h, w, g):   # a gradient buffer of resolution (h, w) that is not g; two per resolution, sized for its widest use
            if (h, w) not in bufs:
                cmax = max(max(ci, co) for (hh, ww, _), (_, ci, co, _) in zip(t.dims, VGG19_LAYOUT) if (hh, ww) == (h, w))
                bufs[(h, w)] = [torch.empty(B * h * w * max(cmax, 32) * esz, dtype=torch.uint8, device=dev) for _ in range(2)]
            a, b = (t.data_ptr() for t in bufs[(h, w)])
            return b if g == a else a

        g = None   # gradient w.r.t. the output F_i of layer i; ReLU mask applied unless layer i is a style or the content tap
        for i in range(len(VGG19_LAYOUT) - 1, -1, -1):
            h, w, c = t.dims[i]
            f, pix = t.acts[i].data_ptr(), h * w * c * esz
            if i in STYLE_TAPS:   # (gF_i + ks (G_b - A_b) F_b) * (F_b > 0): a 1x1 conv per image, gF_i from layer i + 1 as addend
                wgt = torch.zeros(B, c, c, dtype=t.tdt, device=dev)
                self.gw[i] = wgt
                out = other(h, w, g)
                for b in range(B):
                    list_conv(self.bwd_ops, dt, 1, h, w, c, c, 1, f + b * pix, wgt[b].data_ptr(), out + b * pix,
                              addend=(g + b * pix) if g is not None else 0, mask_z=f + b * pix)
                g = out
            elif i == CONTENT_TAP:   # + wc * 2 (F_x - F_c) / n, then the ReLU mask, in place
                self.bwd_ops.add("stl_l2_backward", dt, f, self.ctarget_ptr, g, B * h * w * c, self.cscale.data_ptr(), 1)
            _, ci, co, pool = VGG19_LAYOUT[i]
            out = other(h, w, g)
            if i == 0:   # conv1_1: 1x1 onto the 32-wide patches, then the patch adjoint (with 1 / std) to the NCHW image
                list_conv(self.bwd_ops, dt, B, h, w, co, 32, 1, g, t.wk.data_ptr() + t.tab[0].bwd_off * esz, out)
                self.bwd_ops.add("stl_patch3x3_backward", dt, out, self.dimg.data_ptr(), B, self.H, self.W, 1, mod.std.data_ptr())
                break
            hp, wp, cp = t.dims[i - 1]
            fp = t.acts[i - 1].data_ptr()
            masked = i - 1 not in STYLE_TAPS and i - 1 != CONTENT_TAP   # else the tap masks after adding its own term
            list_conv(self.bwd_ops, dt, B, h, w, co, ci, 3, g, t.wk.data_ptr() + t.tab[i].bwd_off * esz, out,
                      mask_z=fp if masked and not pool else 0)
            if pool:
                dst = other(hp, wp, None)
                self.bwd_ops.add("stl_maxpool2x2_backward", dt, fp, out, dst, B, hp, wp, cp, int(masked))
                out = dst
            g = out

    def backward(self, grams, wc, ws) -> torch.Tensor:
        """Image gradient [B, 3, H, W] fp32 for loss weights wc (content) and ws (style): floats or device scalars.
        grams: per style tap (G [B, C, C], A [B or 1, C, C]) fp64 from the forward pass."""
        B = self.B
        for i, (G, A) in zip(STYLE_TAPS, grams):
            h, w, c = self.trunk.dims[i]
            ks = 4.0 / (B * float(c) ** 3 * h * w)
            self.gw[i].copy_((G - A) * (ws * ks))
        h, w, c = self.trunk.dims[CONTENT_TAP]
        if isinstance(wc, torch.Tensor):
            self.cscale.copy_(wc * (2.0 / (B * h * w * c)))
        else:
            self.cscale.fill_(wc * 2.0 / (B * h * w * c))
        self.bwd_ops.run(torch.cuda.current_stream().cuda_stream)
        return self.dimg


def effective_weights(g_total, g_c, g_s, content_weight: float, style_weight: float):
    """Loss weights (wc, ws) of the content and style terms for the incoming gradients of (total, content, style), with
    total = content_weight * content + style_weight * style: c_loss.backward() alone and total.backward() both come out right."""
    return g_total * content_weight + g_c, g_total * style_weight + g_s


class _Backward:
    """What the backward pass of one forward call needs: the plan (its stored activations), the Gram matrices, the loss weights."""

    def __init__(self, mod, plan, gen, grams):
        self.plan, self.gen, self.grams = plan, gen, grams
        self.cw, self.sw = mod.content_weight, mod.style_weight

    def __call__(self, g_total, g_c, g_s) -> torch.Tensor:
        if self.plan.generation != self.gen:
            raise RuntimeError("VGG19StyleLoss: the module ran forward again on this geometry before this backward; "
                               "call backward() before the next forward")
        wc, ws = effective_weights(g_total, g_c, g_s, self.cw, self.sw)
        return self.plan.backward(self.grams, wc, ws).clone()


class _StyleLossFn(torch.autograd.Function):
    """x -> (total, content, style) with the native image gradient; the losses are computed by the caller's forward launch."""

    @staticmethod
    def forward(ctx, x, losses, bwd):
        ctx.bwd = bwd
        ctx.xdtype = x.dtype
        return tuple(t.detach().clone() for t in losses)

    @staticmethod
    def backward(ctx, g_total, g_c, g_s):
        return ctx.bwd(g_total, g_c, g_s).to(ctx.xdtype), None, None


class VGG19StyleLoss(nn.Module):
    """``VGG19StyleLoss()(stylised, content, style) -> (total, content_loss, style_loss)`` on NCHW images in [0, 1]."""

    def __init__(self, content_weight: float = 1.0, style_weight: float = 1e5, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 compute_dtype: str = "fp32"):
        super().__init__()
        self.content_weight, self.style_weight = float(content_weight), float(style_weight)
        self.dtype = dtype_code(compute_dtype)
        self.features = nn.Module()
        self._convs = [add_conv(self.features, idx, ci, co) for idx, ci, co, _ in VGG19_LAYOUT]
        self.mean = nn.Parameter(torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), requires_grad=False)
        self.std = nn.Parameter(torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1), requires_grad=False)
        self._plans: Dict = {}
        self._flat_dev = None
        if state_dict is not None:
            self.load_state_dict({k: v for k, v in state_dict.items() if k.startswith("features.")}, strict=False)

    def forward(self, x: torch.Tensor, content: torch.Tensor, style: torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("stlpose_amd.VGG19StyleLoss runs only on an MI355X (cuda/HIP device); there is no CPU path")
        dev = x.device
        ready(self, dev)
        st = torch.cuda.current_stream().cuda_stream
        grad = torch.is_grad_enabled() and x.requires_grad
        if grad and (content.requires_grad or style.requires_grad):
            raise NotImplementedError("VGG19StyleLoss differentiates the stylised images only: content and style must not require grad")
        xin = torch.cat([x.detach(), content.detach().to(dev), style.detach().to(dev)], 0).contiguous().float()
        B3, ch, H, W = xin.shape
        if ch != 3 or B3 % 3 or H < 16 or W < 16:
            raise RuntimeError(f"VGG19StyleLoss needs three equal batches of (B, 3, H >= 16, W >= 16) images, got {tuple(xin.shape)}")
        B = B3 // 3
        key = (B3, H, W, grad)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = StylePlan(self, B3, H, W, dev, B, "batch", list(range(B)) + list(range(2 * B, 3 * B)), grad)
        plan.trunk.img.copy_(xin)
        plan.trunk.prep_weights(st)
        plan.trunk.ops.run(st)
        # C x C Gram matrices: split-K slabs -> sum, scale, squared distance (a few hundred KB of bookkeeping)
        s_loss = torch.zeros((), dtype=torch.float64, device=dev)
        grams = []
        for g in plan.grams():
            s_loss = s_loss + ((g[:B] - g[B:]) ** 2).mean()
            grams.append((g[:B], g[B:]))
        s_loss = s_loss.float()
        c_loss = plan.content.clone()
        total = self.content_weight * c_loss + self.style_weight * s_loss
        if not grad:
            return total, c_loss, s_loss
        plan.generation = gen = getattr(plan, "generation", 0) + 1
        return _StyleLossFn.apply(x, (total, c_loss, s_loss), _Backward(self, plan, gen, grams))
