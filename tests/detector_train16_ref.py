"""The yardstick of the 16-bit detector fine-tuning tests: tests/detector_train_ref.method_yardstick restated with a ``store`` hook at
every point where the device rounds (the contract at stl_det_pointwise16_train in include/stlpose_hip.h):

  forward   ``act``: f16 after each depthwise output d, each kept pre-activation z and each swish output t = round(swish(z_unrounded));
            ``wfwd``: the folded pointwise weight W' = W s of the forward MFMA (a header's W' is W);
  backward  ``grad``: bf16 at each stored gradient -- an identity autograd.Function whose backward rounds, placed on every d, every z
            and the two headers' outputs (where it rounds dreg / dlogit); ``wbwd``: the bf16 W'^T of the data gradient; ``xw``: X read
            as bf16 by the weight gradient; swish'(z) is taken from the stored (rounded) z.

The graph keeps detector_train_ref's operations (depthwise conv, 1x1 conv with the raw W and b, eval-mode batch norm, silu) so that
identity stores reproduce it bit for bit; a rounded W' enters as the raw weight W + (store(W s) - W s) / s, which is W exactly under
an identity store and whose fold is store(W s) to within the working precision.  One simplification is stated rather than hidden: the
batch norm's own backward sees the pre-activation made with the forward's rounded W', where the device's fold_chain multiplies dW' by
the unrounded W; the two dgamma differ by the weight rounding (2^-11 per element, averaged over Ci), far inside the bf16 gradient
roundings the emulation carries.  Everything runs in the dtype it is asked for; float64 is the emulation the tests use."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import detector_ref as R
from tests import detector_train_ref as TR


def _ident(t):
    return t


class Stores:
    """The five rounding hooks; the default is the identity everywhere."""

    def __init__(self, act=_ident, wfwd=_ident, wbwd=_ident, xw=_ident, grad=_ident):
        self.act, self.wfwd, self.wbwd, self.xw, self.grad = act, wfwd, wbwd, xw, grad


def rounder(dt):
    """t -> t rounded to dt (round to nearest even), back in t's dtype."""
    return lambda t: t.to(dt).to(t.dtype)


def device_stores() -> Stores:
    """What compute_dtype="f16" rounds: f16 forward tensors and forward weights, bf16 everything the backward stores or stages."""
    h, b = rounder(torch.float16), rounder(torch.bfloat16)
    return Stores(act=h, wfwd=h, wbwd=b, xw=b, grad=b)


class _GradStore(torch.autograd.Function):
    """Identity whose backward rounds: a gradient stored by the device."""

    @staticmethod
    def forward(ctx, x, store):
        ctx.store = store
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.store(g), None


class _ActStore(torch.autograd.Function):
    """A forward tensor as the device stores it; the gradient passes unchanged (the rounding is not differentiated)."""

    @staticmethod
    def forward(ctx, x, store):
        y = store(x)
        return x.view_as(x) if y is x else y

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Swish(torch.autograd.Function):
    """silu(z) of the unrounded z; the backward takes swish'(z) from the stored z."""

    @staticmethod
    def forward(ctx, z, store):
        ctx.save_for_backward(store(z.detach()))
        return F.silu(z.detach())

    @staticmethod
    def backward(ctx, g):
        with torch.enable_grad():
            zs = ctx.saved_tensors[0].detach().requires_grad_(True)
            (gz,) = torch.autograd.grad(F.silu(zs), zs, g)
        return gz, None


class _Pointwise(torch.autograd.Function):
    """conv1x1(x, w + dfwd, b); the data gradient uses w + dbwd, the weight gradient xw(x)."""

    @staticmethod
    def forward(ctx, x, w, b, dfwd, dbwd, xw):
        ctx.save_for_backward(x.detach(), w.detach(), b.detach(), dbwd)
        ctx.xw = xw
        return F.conv2d(x.detach(), w.detach() + dfwd, b.detach())

    @staticmethod
    def backward(ctx, g):
        x, w, b, dbwd = ctx.saved_tensors
        with torch.enable_grad():
            xd = x.detach().requires_grad_(True)
            (gx,) = torch.autograd.grad(F.conv2d(xd, w + dbwd, b), xd, g)
            wd, bd = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
            gw, gb = torch.autograd.grad(F.conv2d(ctx.xw(x), wd, bd), (wd, bd), g)
        return gx, gw, gb, None, None, None


def _delta(w, s, store):
    """The raw-weight perturbation that makes the fold w s equal store(w s); w [co, ci, 1, 1], s [co] or None (no BN: s = 1)."""
    with torch.no_grad():
        if s is None:
            return store(w) - w
        sc = s[:, None, None, None]
        return (store(w * sc) - w * sc) / sc


def _sep(sd, p, x, s, st: Stores):
    """detector_ref._sep(norm=False) with the stores: depthwise (d stored, its gradient stored) then the pointwise layer."""
    c = x.shape[1]
    d = R._conv(sd, p + ".depthwise_conv", x, 3, 1, c)
    d = _GradStore.apply(_ActStore.apply(d, st.act), st.grad)
    w, b = sd[p + ".pointwise_conv.conv.weight"], sd[p + ".pointwise_conv.conv.bias"]
    return _Pointwise.apply(d, w, b, _delta(w, s, st.wfwd), _delta(w, s, st.wbwd), st.xw)


def heads_forward(sd, cc: int, nc: int, levels, st: Stores):
    """detector_train_ref.heads_forward with the stores."""
    from stlpose_amd.efficientdet import HEAD_REPEATS
    outs = []
    for head, k in (("regressor", 4), ("classifier", nc)):
        fs = []
        for lv, f in enumerate(levels):
            for i in range(HEAD_REPEATS[cc]):
                bn = f"{head}.bn_list.{lv}.{i}"
                with torch.no_grad():
                    s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-3)
                z = R._bn(sd, bn, _sep(sd, f"{head}.conv_list.{i}", f, s, st))
                z = _GradStore.apply(z, st.grad)
                f = _ActStore.apply(_Swish.apply(z, st.act), st.act)
            f = _GradStore.apply(_sep(sd, f"{head}.header", f, None, st), st.grad)
            fs.append(f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, k))
        outs.append(torch.cat(fs, 1))
    return outs[0], torch.sigmoid(outs[1])


def method_yardstick(sd, cc, nc, levels, anchors, gt, offsets, dtype, st: Stores = None, **kw):
    """detector_train_ref.method_yardstick through heads_forward above -> (classification, regression, {parameter: grad}, reg, cls,
    N_pos)."""
    st = Stores() if st is None else st
    hs = TR.head_state(sd, dtype)
    reg, cls = heads_forward(hs, cc, nc, [f.detach().cpu().to(dtype) for f in levels], st)
    c, r, npos, _ = TR.detection_loss(reg, cls, anchors, gt, offsets, **kw)
    (c + r).backward()
    grads = {k: v.grad for k, v in hs.items() if v.requires_grad}
    return c.detach(), r.detach(), grads, reg.detach(), cls.detach(), npos
