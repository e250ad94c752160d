"""Yardstick of the split-bf16 conv mode (``stl_conv.math = STL_MATH_BF16X3``, ``compute_dtype="fp32x3"``), test infrastructure only.

An fp32 operand x is split into bf16 pieces, each rounded to nearest even: hi = bf16(x), lo = bf16(x - hi) (and, for the
three-way split, a third piece of what is left).  The device multiplies ``lo*hi + hi*lo + hi*hi`` on the bf16 matrix cores and
accumulates in fp32; ``conv_x3`` is the same three products with every term convolved and summed in fp64, i.e. the value the
device would give with an exact accumulator.  ``bf16x3`` puts that product into every conv of an oracle network.

``LAUNCH_CASES`` / ``launch_case`` are the per-launch shapes, inputs and error bound that tests/test_fp32x3_cpu.py checks on the
host and tests/test_fp32x3_gpu.py holds the kernels to.
"""
from __future__ import annotations

import functools
import types

import torch
import torch.nn as nn
import torch.nn.functional as F


def split_bf16(t: torch.Tensor, pieces: int = 2):
    """The `pieces` bf16 pieces of an fp32 tensor, largest first, as fp32 tensors (round to nearest even at every step)."""
    t = t.float()
    out = []
    for _ in range(pieces):
        p = t.to(torch.bfloat16).float()
        out.append(p)
        t = t - p
    return out


def conv_x3(x: torch.Tensor, w: torch.Tensor, stride=1, padding=0, bias=None, drop_lo_hi: bool = False) -> torch.Tensor:
    """w_lo*x_hi + w_hi*x_lo + w_hi*x_hi, each term convolved in fp64; fp64 result (+ bias).  drop_lo_hi: without the first
    term (what a two-product kernel would compute)."""
    (xh, xl), (wh, wl) = split_bf16(x), split_bf16(w)
    c = lambda a, b: F.conv2d(a.double(), b.double(), None, stride, padding)   # noqa: E731
    y = c(xl, wh) + c(xh, wh)
    if not drop_lo_hi:
        y = c(xh, wl) + y
    return y if bias is None else y + bias.double().view(1, -1, 1, 1)


def conv_x3_fp32(x: torch.Tensor, w: torch.Tensor, stride=1, padding=0) -> torch.Tensor:
    """The same three products evaluated and summed in fp32, smallest first: an accumulator like the device's."""
    (xh, xl), (wh, wl) = split_bf16(x), split_bf16(w)
    c = lambda a, b: F.conv2d(a, b, None, stride, padding)   # noqa: E731
    return (c(xh, wl) + c(xl, wh)) + c(xh, wh)


class bf16x3:
    """Context manager in the style of ``oracle.hrnet_ref.bf16_storage``: inside it every ``nn.Conv2d`` of `model` except
    ``final_layer`` (the head is not a conv launch on the device) computes ``conv_x3``, rounded to its input's dtype.  `model` may
    also be the module ``oracle.vgg_ref``, whose VGG16 restatement calls ``F.conv2d`` directly: its ``F`` is swapped for a
    namespace whose ``conv2d`` is ``conv_x3``.  Everything is put back on exit."""

    def __init__(self, model):
        self.model, self.saved = model, []

    def __enter__(self):
        m = self.model
        if isinstance(m, types.ModuleType):
            real = m.F
            shim = types.SimpleNamespace(**{k: getattr(real, k) for k in dir(real) if not k.startswith("__")})
            shim.conv2d = lambda x, w, bias=None, stride=1, padding=0: conv_x3(x, w, stride, padding, bias).to(x.dtype)
            self.saved.append((m, "F", real))
            m.F = shim
            return m
        for name, mod in m.named_modules():
            if isinstance(mod, nn.Conv2d) and name != "final_layer":
                assert mod.groups == 1 and mod.dilation == (1, 1) and mod.padding_mode == "zeros"
                self.saved.append((mod, "forward", mod.__dict__.get("forward")))
                mod.forward = functools.partial(self._forward, mod)
        return m

    @staticmethod
    def _forward(mod, x):
        return conv_x3(x, mod.weight, mod.stride, mod.padding, mod.bias).to(x.dtype)

    def __exit__(self, *exc):
        for obj, attr, old in self.saved:
            if old is None:
                delattr(obj, attr)   # the instance attribute that shadowed the class's forward
            else:
                setattr(obj, attr, old)
        self.saved = []
        return False


# ---------------------------------------------------------------------------------------- per-launch cases
# (name, B, H, W, Ci, Co, ks, stride, real Ci): the smallest shapes at which each path of the kernels can go wrong.
#   * stem: the stem conv is launched as a 1x1 conv over 32-wide 3x3 patches of which 27 channels are real -- the tensor and the
#     filters carry zeros in channels 27..31 (stl_conv needs Ci % 4 == 0), so the second K chunk is half padding.
#   * ragged: stl_conv needs Co % 8 == 0, so the ragged case has 40 output channels (2.5 channel tiles), not 36.
LAUNCH_CASES = [
    ("c32", 2, 12, 9, 32, 32, 3, 1, 32),        # virtual rows, filters LDS-resident per chunk
    ("stride2", 2, 12, 10, 32, 64, 3, 2, 32),   # stride 2: the wave-specialised kernel
    ("stream1x1", 2, 8, 6, 64, 256, 1, 1, 64),  # streaming path 0
    ("stem", 2, 16, 12, 32, 64, 1, 1, 27),      # K = 27 of 32
    ("tiny", 2, 8, 6, 4, 8, 3, 1, 4),           # the tiny net: tiles mostly padding
    ("deep", 2, 12, 9, 256, 256, 3, 1, 256),    # several K chunks, filters staged per chunk
    ("ragged", 3, 7, 5, 20, 40, 3, 1, 20),      # everything ragged
]
MARGIN, FLOOR = 8.0, 1e-6   # tests/test_vgg_layers_gpu.py's: a launch may be MARGIN x the fp32 conv's own error away, at least FLOOR


def case_tensors(name: str):
    """(x NCHW, w OIHW, stride, padding) of a case: x = relu(1.3 randn + 0.2), He-normal weights, fixed seed."""
    _, B, H, W, Ci, Co, ks, stride, real = next(c for c in LAUNCH_CASES if c[0] == name)
    g = torch.Generator().manual_seed(20240 + [c[0] for c in LAUNCH_CASES].index(name))
    x = torch.relu(1.3 * torch.randn(B, Ci, H, W, generator=g) + 0.2)
    w = torch.randn(Co, Ci, ks, ks, generator=g) * (2.0 / (real * ks * ks)) ** 0.5
    x[:, real:], w[:, real:] = 0.0, 0.0
    return x, w, stride, ks // 2


def bound_for(x, w, stride, padding, bias=None, relu: bool = False):
    """(Y fp64, bound): Y = conv_x3 (+ bias, ReLU), bound = max(MARGIN * e32, FLOOR) with e32 the distance of the fp32 conv from
    the fp64 conv relative to max |Y| -- what plain fp32 accumulation costs on these very operands."""
    act = torch.relu if relu else (lambda t: t)
    y = act(conv_x3(x, w, stride, padding, bias))
    y32 = act(F.conv2d(x, w, bias, stride, padding)).double()
    y64 = act(F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride, padding))
    e32 = float((y32 - y64).abs().max() / y.abs().max())
    return y, max(MARGIN * e32, FLOOR)


@functools.lru_cache(maxsize=None)
def launch_case(name: str):
    """(x, w, stride, padding, Y, bound) of a case, computed once per process and shared (callers must not write to them)."""
    x, w, stride, padding = case_tensors(name)
    return (x, w, stride, padding) + bound_for(x, w, stride, padding)
