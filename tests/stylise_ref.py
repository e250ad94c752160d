"""Test helpers for the VGG19 image gradient and the Gatys driver (stlpose_amd/stylise.py): restatements on torch CPU of
autograd of ``oracle.vgg_ref`` and of the closed forms the native backward implements.  Pure torch: no GPU, no product code."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import vgg_ref

TAPS, CTAP = vgg_ref.VGG19_STYLE_TAPS, vgg_ref.VGG19_CONTENT_TAP


def normalise(x: torch.Tensor) -> torch.Tensor:
    mean = torch.tensor(vgg_ref.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(vgg_ref.IMAGENET_STD).view(1, 3, 1, 1)
    return (x - mean) / std


def oracle_image_grad(x, content, style, weights, cw, sw, which="total", dtype=torch.float32):
    """x.grad of output `which` ("total", "content", "style" or a (a, b, c) weighting) by autograd of the oracle loss."""
    w = {k: v.to(dtype) for k, v in weights.items()}
    xs = x.detach().to(dtype).requires_grad_(True)
    tot, c, s = vgg_ref.vgg19_style_content_loss(xs, content.to(dtype), style.to(dtype), w, cw, sw)
    if isinstance(which, tuple):
        out = which[0] * tot + which[1] * c + which[2] * s
    else:
        out = {"total": tot, "content": c, "style": s}[which]
    out.backward()
    return xs.grad.float(), (tot.item(), c.item(), s.item())


def gram_tap_grad(f: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """Closed form of d/dF of mse(gram(F), A) over the batch: 4 / (B C^3 HW) (G_b - A_b) F_b."""
    b, c, h, w = f.shape
    m = f.reshape(b, c, h * w)
    g = torch.bmm(m, m.transpose(1, 2)) / (c * h * w)
    return (4.0 / (b * c ** 3 * h * w) * torch.bmm(g - a, m)).reshape(f.shape)


def content_tap_grad(fx: torch.Tensor, fc: torch.Tensor) -> torch.Tensor:
    """Closed form of d/dF_x of mse(F_x, F_c): 2 (F_x - F_c) / n."""
    return 2.0 * (fx - fc) / fx.numel()


def maxpool_backward_restated(x: torch.Tensor, dy: torch.Tensor, mask: bool) -> torch.Tensor:
    """2x2 / stride-2 max-pool adjoint in the gather form of stl_maxpool2x2_backward, on NCHW: each window's gradient goes to its
    first maximum in row-major order (later elements win only if strictly greater, or NaN); dropped edge rows / columns get 0;
    mask: also 0 where x <= 0."""
    B, C, H, W = x.shape
    dx = torch.zeros_like(x)
    for wy in range(H // 2):
        for wx in range(W // 2):
            win = x[:, :, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2].reshape(B, C, 4)
            m, idx = win[:, :, 0].clone(), torch.zeros(B, C, dtype=torch.long)
            for k in range(1, 4):
                take = (win[:, :, k] > m) | torch.isnan(win[:, :, k])
                m = torch.where(take, win[:, :, k], m)
                idx = torch.where(take, torch.full_like(idx, k), idx)
            for k in range(4):
                v = torch.where(idx == k, dy[:, :, wy, wx], torch.zeros_like(m))
                if mask:
                    v = torch.where(win[:, :, k] > 0, v, torch.zeros_like(v))
                dx[:, :, 2 * wy + k // 2, 2 * wx + k % 2] = v
    return dx


def cached_targets(content, style, weights):
    """relu4_2 features of `content` and the style Grams per style tap (style: 1 or B images of any size)."""
    with torch.no_grad():
        fc = vgg_ref.vgg19_taps(normalise(content), weights)[CTAP]
        fs = vgg_ref.vgg19_taps(normalise(style), weights)
        return fc, [vgg_ref.gram(fs[i]) for i in TAPS]


def cached_loss(x, fc, grams, weights, cw, sw):
    f = vgg_ref.vgg19_taps(normalise(x), weights)
    c = F.mse_loss(f[CTAP], fc)
    s = sum(((vgg_ref.gram(f[i]) - a) ** 2).mean() for i, a in zip(TAPS, grams))
    return cw * c + sw * s


def oracle_stylise_sgd(content, style, weights, cw, sw, steps, lr, clamp=True):
    """The cached-target Gatys loop with torch.optim.SGD on the oracle (CPU fp32): (image, per-step losses before each step)."""
    fc, grams = cached_targets(content, style, weights)
    img = content.clone().requires_grad_(True)
    opt = torch.optim.SGD([img], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = cached_loss(img, fc, grams, weights, cw, sw)
        loss.backward()
        losses.append(loss.item())
        opt.step()
        if clamp:
            with torch.no_grad():
                img.clamp_(0.0, 1.0)
    return img.detach(), losses
