"""Gatys et al. (2016) stylisation on MI355X: descend the VGG19 content + Gram style loss (``vgg19_style.py``) with respect to
the image -- the "VGG19 stylise" step of BASELINE config 5 (Styled-COCO: stylise, then fine-tune HRNet-W32).

No reference counterpart: PARITY UNPINNED; checked against torch autograd of
``oracle.vgg_ref.vgg19_style_content_loss``.

The content features at relu4_2 and the style images' Gram matrices are computed ONCE per call.  Every iteration then runs the
VGG19 forward (up to conv5_1) and the native image gradient on the B stylised images only -- a third of the work of a
``VGG19StyleLoss`` call on (stylised, content, style) -- and a ``torch.optim`` step on a device leaf tensor.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .vgg import ready
from .vgg19_style import CONTENT_TAP, StylePlan, VGG19StyleLoss

OPTIMIZERS = ("adam", "lbfgs", "sgd")


class GatysStylizer:
    """``GatysStylizer(state_dict)(content, style, steps, lr)`` -> stylised NCHW images in [0, 1].

    content: (B, 3, H, W) images in [0, 1]; style: 1 image (used for every content image) or B images, of any size >= 16
    (it need not match the content's).  The loss is content_weight * mse(relu4_2) + style_weight * sum of the Gram MSEs at
    relu1_1 .. relu5_1, as ``VGG19StyleLoss``.  ``losses`` holds the loss before each step of the last call."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], content_weight: float = 1.0, style_weight: float = 1e5,
                 compute_dtype: str = "fp32"):
        self.loss = VGG19StyleLoss(content_weight, style_weight, state_dict=state_dict, compute_dtype=compute_dtype)
        self.content_weight, self.style_weight = self.loss.content_weight, self.loss.style_weight
        self._plans: Dict = {}
        self.losses: List[float] = []

    # ---------------------------------------------------------------- plans and targets
    def _plan(self, dev, nb, H, W, content: Optional[str], grad: bool) -> StylePlan:
        key = (nb, H, W, content, grad)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = StylePlan(self.loss, nb, H, W, dev, nb, content, list(range(nb)), grad)
            plan.trunk.prep_weights(torch.cuda.current_stream().cuda_stream)
        return plan

    def targets(self, content: torch.Tensor, style: torch.Tensor):
        """(iteration plan with the relu4_2 features of `content` cached in it, style Grams [Bs, C, C] fp64 per tap)."""
        dev = content.device
        B, _, H, W = content.shape
        st = torch.cuda.current_stream().cuda_stream
        it = self._plan(dev, B, H, W, "buffer", True)
        it.trunk.img.copy_(content)
        it.trunk.ops.run(st)
        it.ctarget.view(torch.uint8).copy_(it.trunk.acts[CONTENT_TAP])
        Bs, _, Hs, Ws = style.shape
        sp = self._plan(dev, Bs, Hs, Ws, None, False)
        sp.trunk.img.copy_(style)
        sp.trunk.ops.run(st)
        return it, sp.grams()

    # ---------------------------------------------------------------- one iteration, in two halves (tools/stylise_bench.py times them)
    def forward_loss(self, it: StylePlan, img: torch.Tensor, style_grams):
        """Forward of the B images `img` against the cached targets: (total loss, per-tap (G, A)) on device."""
        it.trunk.img.copy_(img)
        it.trunk.ops.run(torch.cuda.current_stream().cuda_stream)
        s_loss = torch.zeros((), dtype=torch.float64, device=img.device)
        grams = []
        for G, A in zip(it.grams(), style_grams):
            s_loss = s_loss + ((G - A) ** 2).mean()
            grams.append((G, A))
        return self.content_weight * it.content + self.style_weight * s_loss.float(), grams

    def image_grad(self, it: StylePlan, grams) -> torch.Tensor:
        """d total / d img [B, 3, H, W] fp32 of the last forward_loss (a buffer of the plan, overwritten by the next call)."""
        return it.backward(grams, self.content_weight, self.style_weight)

    # ---------------------------------------------------------------- driver
    def stylise(self, content: torch.Tensor, style: torch.Tensor, steps: int = 100, lr: float = 0.05, optimizer: str = "adam",
                init: str = "content", clamp: bool = True) -> torch.Tensor:
        if not content.is_cuda:
            raise RuntimeError("stlpose_amd.GatysStylizer runs only on an MI355X (cuda/HIP device); there is no CPU path")
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        if init not in ("content", "noise"):
            raise ValueError(f"init must be 'content' or 'noise', got {init!r}")
        dev = content.device
        content = content.detach().to(dev).float().contiguous()
        style = style.detach().to(dev).float().contiguous()
        if style.dim() == 3:
            style = style.unsqueeze(0)
        B, ch, H, W = content.shape
        if ch != 3 or H < 16 or W < 16:
            raise RuntimeError(f"GatysStylizer: content must be (B, 3, H >= 16, W >= 16), got {tuple(content.shape)}")
        if style.shape[1] != 3 or style.shape[0] not in (1, B) or min(style.shape[2:]) < 16:
            raise RuntimeError(f"GatysStylizer: style must be 1 or {B} images (3, H >= 16, W >= 16), got {tuple(style.shape)}")
        ready(self.loss, dev)
        it, style_grams = self.targets(content, style)
        img = (content.clone() if init == "content" else torch.rand_like(content)).requires_grad_(True)
        img.grad = torch.zeros_like(img)
        if optimizer == "adam":
            opt = torch.optim.Adam([img], lr=lr)
        elif optimizer == "sgd":
            opt = torch.optim.SGD([img], lr=lr)
        else:
            opt = torch.optim.LBFGS([img], lr=lr, max_iter=20, history_size=50)

        def closure():
            loss, grams = self.forward_loss(it, img.detach(), style_grams)
            img.grad.copy_(self.image_grad(it, grams))
            return loss

        losses = []
        for _ in range(steps):
            losses.append(opt.step(closure))
            if clamp:
                with torch.no_grad():
                    img.clamp_(0.0, 1.0)
        self.losses = [float(t) for t in losses]
        return img.detach()

    __call__ = stylise
