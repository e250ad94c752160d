"""The yardstick of the VGG trunk's layer-by-layer tests (tests/test_vgg_layers_cpu.py, test_vgg_layers_gpu.py, test_vgg_ops_gpu.py):
one trunk layer restated in plain torch, the two error bounds, and the image cases the GPU tests run.  CPU only: nothing here
touches the HIP library.

One layer is ``relu(conv2d(maxpool2x2_floor(x_prev) if pool else x_prev, w, b, padding=1))``, evaluated in float64 (the yardstick)
or float32 (the eager evaluation whose own error scales the bounds).  Chained in float32 it is ``oracle.vgg_ref.vgg_features`` /
``vgg19_taps`` bit for bit (tests/test_vgg_layers_cpu.py), which ties it to the oracle pinned by fixture G10.

Bounds.  ``rel_err(got, y64) = max|got - y64| / max|y64|``.
* ``hold`` (fp32 tensors, and fp32 results formed from exactly known inputs): ``e <= max(MARGIN * e32, FLOOR)`` with e32 the same
  figure of the fp32 torch evaluation -- the convention of tests/test_detector_train_gpu.py, whose FLOOR (1e-6) is used as it is.
  MARGIN is that file's 8: a kernel adds the products of a Gram entry or a reduction in another order than torch does (MFMA tiles,
  split-K slabs, fp64 partial sums), the same situation as there.
* MARGIN_CONV32 = 16, for the fp32 3x3 convs only.  With u = 2**-24 = 6e-8, torch's own e32 stays at 2u .. 12u (1.2e-7 .. 7.0e-7,
  typically 4u) from K = 27 to K = 9 * 512 = 4608 products per output: its blocked accumulation hardly grows with K.  A kernel
  that carries ONE fp32 accumulator through all K / 2 MFMA steps -- a legitimate order -- has a random-walk rounding error of about
  u * sqrt(K) / 2 at the largest outputs: 34u = 2.0e-6 at K = 4608, eight times torch's typical e32 before the maximum over a
  tensor's elements is taken, so 8 cannot hold for a correct kernel there; 16 is the next power of two.  (Measured on the MI355X,
  e grows as that model says: e <= 1.2e-6 / 1.3e-6 / 2.1e-6 / 2.4e-6 and e / e32 <= 4.3 / 5.5 / 7.9 / 9.0 at K = 576 / 1152 / 2304 /
  4608; a fault does not scale with sqrt(K).)  tests/test_vgg_layers_cpu.py rejects every seeded fault at this margin.
* ``hold16`` (tensors stored in a 16-bit type), for EVERY element: ``|got - y64| <= r * |y64| + max(MARGIN * e32, FLOOR) * max|y64|``
  with r = 2**-8 for bf16: one unit in the last place of its 7 stored fraction bits, relative to the binade's upper end, which is
  also the largest relative error of one round-to-nearest (half a unit at the binade's lower end); f16: 2**-11.  The second
  term is ``hold``'s bound on the fp32 value that is rounded, and lets the rounding flip where that value sits on a tie.
"""
from __future__ import annotations

import zlib

import torch
import torch.nn.functional as F

from oracle import vgg_ref
from tests.detector_train_ref import FLOOR, rel_err  # noqa: F401  (re-exported)

MARGIN = 8.0
MARGIN_CONV32 = 16.0
ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# (features index, 2x2 max-pool in front) per conv, in trunk order
VGG16_ROWS = []
for _ops in vgg_ref.VGG16_SLICES:
    _pool = False
    for _op in _ops:
        if _op == "p":
            _pool = True
        else:
            VGG16_ROWS.append((vgg_ref.VGG16_CONVS[int(_op[1:])][0], _pool))
            _pool = False
VGG16_SLICE_END = (1, 3, 6, 9)   # conv positions after which a slice ends
VGG19_ROWS = [(idx, pool) for idx, _, _, pool in vgg_ref.VGG19_CONVS]

# the image shapes of the GPU tests: the smallest that still exercise the edges (tests/test_vgg_layers_cpu.py asserts what they
# have).  VGG16: input and target of B images each; VGG19: stylised, content and style of B images each.
VGG16_CASES = {
    "44x36": dict(B=2, C=3, H=44, W=36, resize=False),    # pool inputs 44/22/11 x 36/18/9: odd in both axes
    "8x8": dict(B=2, C=3, H=8, W=8, resize=False),        # the minimum: the last maps are 1 x 1
    "9x11": dict(B=2, C=3, H=9, W=11, resize=False),      # the floor drops a row and a column at the first pool
    "gray224": dict(B=1, C=1, H=40, W=56, resize=True),   # channel repeat + bilinear to 224 x 224
}
VGG19_CASES = {
    "2x44x36": dict(B=2, H=44, W=36),                     # last map 2 x 2
    "1x16x16": dict(B=1, H=16, W=16),                     # the minimum: last map 1 x 1
    "2x17x19": dict(B=2, H=17, W=19),
}


def case_images(net: str, name: str, run: int = 0):
    """The images of one case in [0, 1]: (input, target) for "vgg16", (stylised, content, style) for "vgg19"; run 1 gives
    different images of the same shape (the stale-plan check)."""
    case = (VGG16_CASES if net == "vgg16" else VGG19_CASES)[name]
    g = torch.Generator().manual_seed((zlib.crc32(f"{net}.{name}".encode()) + 7919 * run) & 0x7FFFFFFF)
    shape = (case["B"], case.get("C", 3), case["H"], case["W"])
    return tuple(torch.rand(*shape, generator=g) for _ in range(2 if net == "vgg16" else 3))


def normalise(img: torch.Tensor, dtype) -> torch.Tensor:
    """(img - mean) / std in `dtype`; mean and std are the fp32 constants the modules hold, converted exactly."""
    mean = torch.tensor(vgg_ref.IMAGENET_MEAN).view(1, 3, 1, 1).to(dtype)
    std = torch.tensor(vgg_ref.IMAGENET_STD).view(1, 3, 1, 1).to(dtype)
    return (img.to(dtype) - mean) / std


def layer(x_prev: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, pool: bool, dtype, bf16_weights: bool = False) -> torch.Tensor:
    """One trunk layer from its NCHW input, in `dtype` (torch.float64 or torch.float32).  bf16_weights: the weights are rounded
    to bf16 first, as stl_weight_prep does for a bf16 plan; the bias stays fp32 in both modes, as in Trunk."""
    w = weight.bfloat16() if bf16_weights else weight
    x = x_prev.to(dtype)
    if pool:
        x = F.max_pool2d(x, 2, 2)
    return F.relu(F.conv2d(x, w.to(dtype), bias.to(dtype), padding=1))


def unfold3x3(x: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """NCHW (3 channels) -> the 3x3 pad-1 patches [B, Ho, Wo, 27] in stl_patch3x3's column order (ky * 3 + kx) * 3 + c."""
    b, c, h, w = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    u = F.unfold(x, 3, padding=1, stride=stride)   # [B, c * 9 + tap, Ho * Wo]
    return u.view(b, c, 9, ho, wo).permute(0, 3, 4, 2, 1).reshape(b, ho, wo, 9 * c)


def patch_layer(patches: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, dtype, bf16_weights: bool = False) -> torch.Tensor:
    """conv1_1 as the trunk runs it: the 1x1 conv of the stored patches [B, H, W, 27] with the [Co, 27] weights, bias, ReLU ->
    NCHW.  On the patches of x it is layer(x, ...) up to the order of the 27 additions."""
    w = weight.bfloat16() if bf16_weights else weight
    w27 = w.to(dtype).permute(0, 2, 3, 1).reshape(w.shape[0], 27)
    return F.relu(patches.to(dtype) @ w27.t() + bias.to(dtype)).permute(0, 3, 1, 2).contiguous()


def gram(f: torch.Tensor, dtype) -> torch.Tensor:
    """NCHW features -> [B, C, C] Gram matrices F F^T / (C H W) in `dtype`."""
    b, c, h, w = f.shape
    m = f.to(dtype).reshape(b, c, h * w)
    return torch.bmm(m, m.transpose(1, 2)) / (c * h * w)


def bound(e32: float, margin: float = MARGIN) -> float:
    return max(margin * e32, FLOOR)


def hold(name: str, got, y64, y32, margin: float = MARGIN) -> float:
    """Print the figures, then hold e to max(margin * e32, FLOOR).  Returns e / e32."""
    e, e32 = rel_err(got, y64), rel_err(y32, y64)
    ratio = e / e32 if e32 else float("inf")
    print(f"{name}: e {e:.3e} e32 {e32:.3e} ratio {ratio:.2f}")
    assert e <= bound(e32, margin), (name, e, e32)
    return ratio


def hold16(name: str, got, y64, y32, ulp: float = ROUND[torch.bfloat16]) -> float:
    """The elementwise bound of a tensor stored in a 16-bit type: no exclusions.  Returns the largest |got - y64| / allowed."""
    got, y64 = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(y64).detach().cpu().double()
    assert got.shape == y64.shape, (got.shape, y64.shape)
    e32 = rel_err(y32, y64)
    top = y64.abs().max().item() if y64.numel() else 0.0
    allowed = ulp * y64.abs() + bound(e32) * top
    err = (got - y64).abs()
    worst = (err / allowed.clamp(min=1e-300)).max().item() if y64.numel() else 0.0
    e = err.max().item() / top if top > 0 else err.max().item()
    print(f"{name}: e {e:.3e} e32 {e32:.3e} ratio {e / e32 if e32 else float('inf'):.2f} worst/allowed {worst:.3f}")
    bad = ~(err <= allowed)   # a NaN fails
    assert not bad.any(), (name, int(bad.sum()), worst, e32)
    return worst
