"""Yardstick of ``stlpose_amd.adain``: the published AdaIN network (Huang & Belongie 2017) restated in plain PyTorch -- the two
``nn.Sequential``s of the published weight files with ``nn.ReflectionPad2d``, ``nn.MaxPool2d(ceil_mode=True)``,
``nn.Upsample(nearest)`` and ``Tensor.var``.  CPU, any dtype; no product code.  There is no reference item for the stylizer
(PARITY UNPINNED): this file is what the tests compare against.  Weights are synthetic, from a fixed seed."""
from __future__ import annotations

import copy
from typing import Optional

import torch
import torch.nn as nn

EPS = 1e-5


def encoder() -> nn.Sequential:
    """The "normalised VGG19" up to relu4_1: 31 entries, convs at 0 (1x1), 2, 5, 9, 12, 16, 19, 22, 25, 29."""
    layers = [nn.Conv2d(3, 3, 1)]
    for c in [(3, 64), (64, 64), "P", (64, 128), (128, 128), "P", (128, 256), (256, 256), (256, 256), (256, 256), "P", (256, 512)]:
        if c == "P":
            layers.append(nn.MaxPool2d(2, 2, 0, ceil_mode=True))
        else:
            layers += [nn.ReflectionPad2d(1), nn.Conv2d(c[0], c[1], 3), nn.ReLU()]
    return nn.Sequential(*layers)


def decoder() -> nn.Sequential:
    """29 entries, convs at 1, 5, 8, 11, 14, 18, 21, 25, 28, nearest x2 upsampling at 3, 16, 23, no ReLU after the last conv."""
    cfg = [(512, 256), "U", (256, 256), (256, 256), (256, 256), (256, 128), "U", (128, 128), (128, 64), "U", (64, 64), (64, 3)]
    layers = []
    for i, c in enumerate(cfg):
        if c == "U":
            layers.append(nn.Upsample(scale_factor=2, mode="nearest"))
        else:
            layers += [nn.ReflectionPad2d(1), nn.Conv2d(c[0], c[1], 3)]
            if i != len(cfg) - 1:
                layers.append(nn.ReLU())
    return nn.Sequential(*layers)


def synth(seed: int = 0):
    """(encoder, decoder) with Kaiming-normal weights and N(0, 0.1) biases from a fixed seed, in eval mode."""
    g = torch.Generator().manual_seed(seed)
    enc, dec = encoder(), decoder()
    with torch.no_grad():
        for m in list(enc) + list(dec):
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)   # kaiming_normal_, fan_in, ReLU gain
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    for p in list(enc.parameters()) + list(dec.parameters()):
        p.requires_grad_(False)
    return enc.eval(), dec.eval()


def mean_sigma(f: torch.Tensor, eps: float = EPS):
    """Per (image, channel) mean and sqrt(unbiased variance + eps) over the pixels, [B, C, 1, 1] each."""
    B, C = f.shape[:2]
    flat = f.reshape(B, C, -1)
    return flat.mean(2).view(B, C, 1, 1), (flat.var(2) + eps).sqrt().view(B, C, 1, 1)


def adain(fc: torch.Tensor, ms: torch.Tensor, ss: torch.Tensor, alpha: float) -> torch.Tensor:
    """The two-step form: normalise and re-style, then blend with the content features."""
    mc, sc = mean_sigma(fc)
    t = ss * (fc - mc) / sc + ms
    return alpha * t + (1 - alpha) * fc


def style_stats(enc: nn.Sequential, style: torch.Tensor, B: int, style_weights: Optional[torch.Tensor] = None, rnd=lambda t: t):
    """(mean, sigma) [B, C, 1, 1] of the style for each of the B content images: one style for all, one per image, or the
    published interpolation sum_k w[b, k] * (mean_k, sigma_k)."""
    ms, ss = mean_sigma(run_seq(enc, style, rnd))
    if style_weights is not None:
        w = style_weights.to(ms.dtype)
        return (w @ ms.flatten(1)).view(B, -1, 1, 1), (w @ ss.flatten(1)).view(B, -1, 1, 1)
    if ms.shape[0] == 1:
        return ms.expand(B, -1, -1, -1), ss.expand(B, -1, -1, -1)
    return ms, ss


def run_seq(seq: nn.Sequential, x: torch.Tensor, rnd=lambda t: t) -> torch.Tensor:
    """seq(x), with `rnd` applied to every map a kernel would store (after each ReLU and after the last conv)."""
    n = len(seq)
    for i, m in enumerate(seq):
        x = m(x)
        if isinstance(m, nn.ReLU) or i == n - 1:
            x = rnd(x)
    return x


@torch.no_grad()
def stylise(enc: nn.Sequential, dec: nn.Sequential, content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0,
            style_weights: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """decoder(alpha * adain(encoder(content), encoder(style)) + (1 - alpha) * encoder(content)) in `dtype`."""
    enc, dec = copy.deepcopy(enc).to(dtype), copy.deepcopy(dec).to(dtype)
    fc = enc(content.to(dtype))
    ms, ss = style_stats(enc, style.to(dtype), content.shape[0], style_weights)
    return dec(adain(fc, ms, ss, alpha))


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


@torch.no_grad()
def stylise_bf16_rounded(enc: nn.Sequential, dec: nn.Sequential, content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0):
    """The yardstick of the bf16 mode: the same network in fp32 arithmetic with its weights, its input images and every stored
    map (each post-ReLU map, the transformed features, the last conv's output) rounded to bf16.  Biases, statistics and the
    affine stay fp32, as a bf16 kernel with fp32 accumulation keeps them."""
    enc, dec = copy.deepcopy(enc), copy.deepcopy(dec)
    for m in list(enc) + list(dec):
        if isinstance(m, nn.Conv2d):
            m.weight.copy_(_bf16(m.weight))
    fc = run_seq(enc, _bf16(content), _bf16)
    ms, ss = style_stats(enc, _bf16(style), content.shape[0], None, _bf16)
    return run_seq(dec, _bf16(adain(fc, ms, ss, alpha)), _bf16)


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def cosine(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()))
