"""CPU: the closed forms behind the native VGG19 image gradient (stlpose_amd/vgg19_style.py) and the Gatys driver
(stlpose_amd/stylise.py), checked against torch autograd of oracle.vgg_ref.  PARITY UNPINNED (no reference counterpart)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import vgg_ref
from stlpose_amd import GatysStylizer, VGG19StyleLoss  # noqa: F401
from stlpose_amd.vgg19_style import CONTENT_TAP, STYLE_TAPS, effective_weights

from tests import stylise_ref as R


def _taps(seed, B=2, H=40, W=36):
    g = torch.Generator().manual_seed(seed)
    w = vgg_ref.synth_vgg19_weights()
    return vgg_ref.vgg19_taps(R.normalise(torch.rand(B, 3, H, W, generator=g)), w), g


def test_tap_constants_match_oracle():
    assert STYLE_TAPS == vgg_ref.VGG19_STYLE_TAPS and CONTENT_TAP == vgg_ref.VGG19_CONTENT_TAP


@pytest.mark.parametrize("tap", vgg_ref.VGG19_STYLE_TAPS)
def test_gram_closed_form_matches_autograd(tap):
    f, _ = _taps(1)
    f = f[tap].double()
    b, c = f.shape[:2]
    a = vgg_ref.gram(_taps(4, H=28, W=52)[0][tap].double())   # a style Gram: symmetric, any image size
    fl = f.clone().requires_grad_(True)
    F.mse_loss(vgg_ref.gram(fl), a).backward()
    ref = fl.grad
    got = R.gram_tap_grad(f, a)
    assert torch.allclose(got, ref, rtol=1e-10, atol=1e-14 * ref.abs().max().item())
    # a broadcast single style Gram is the same as B copies of it
    a1 = a[:1]
    fl.grad = None
    ((vgg_ref.gram(fl) - a1) ** 2).mean().backward()
    assert torch.allclose(R.gram_tap_grad(f, a1.expand(b, c, c)), fl.grad, rtol=1e-10, atol=1e-14 * fl.grad.abs().max().item())


def test_content_closed_form_matches_autograd():
    fx, _ = _taps(2)
    fc, _ = _taps(3)
    fx, fc = fx[CONTENT_TAP].double(), fc[CONTENT_TAP].double()
    fl = fx.clone().requires_grad_(True)
    F.mse_loss(fl, fc).backward()
    assert torch.allclose(R.content_tap_grad(fx, fc), fl.grad, rtol=1e-12, atol=0)


@pytest.mark.parametrize("gt,gc,gs", [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, -2.0, 3.0)])
def test_effective_weights_match_autograd(gt, gc, gs):
    cw, sw = 0.7, 1e3
    theta = torch.tensor([0.3, -1.2], dtype=torch.float64, requires_grad=True)
    c = (theta ** 2).sum()           # stand-ins for the content and style losses as functions of the image
    s = torch.sin(theta).prod()
    total = cw * c + sw * s
    (gt * total + gc * c + gs * s).backward()
    dc = torch.autograd.functional.jacobian(lambda t: (t ** 2).sum(), theta.detach())
    ds = torch.autograd.functional.jacobian(lambda t: torch.sin(t).prod(), theta.detach())
    wc, ws = effective_weights(torch.tensor(gt, dtype=torch.float64), torch.tensor(gc, dtype=torch.float64),
                               torch.tensor(gs, dtype=torch.float64), cw, sw)
    assert torch.allclose(wc * dc + ws * ds, theta.grad, rtol=1e-12)


@pytest.mark.parametrize("H,W", [(8, 6), (7, 9), (5, 5), (2, 3)])
@pytest.mark.parametrize("mask", [False, True])
def test_maxpool_adjoint_restatement_matches_torch(H, W, mask):
    g = torch.Generator().manual_seed(H * 31 + W)
    z = torch.randint(-1, 3, (2, 8, H, W), generator=g).float()   # few levels: ties in most windows, all-zero windows too
    zl = z.clone().requires_grad_(True)
    x = F.relu(zl) if mask else zl
    y = F.max_pool2d(x, 2, 2)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    got = R.maxpool_backward_restated(F.relu(z) if mask else z, dy, mask)
    assert torch.equal(got, zl.grad)
    if H % 2:
        assert (got[:, :, -1] == 0).all()
    if W % 2:
        assert (got[:, :, :, -1] == 0).all()


def test_cpu_tensors_raise_no_cpu_path():
    w = vgg_ref.synth_vgg19_weights()
    x = torch.rand(1, 3, 32, 32, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        VGG19StyleLoss(state_dict=w)(x, torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        GatysStylizer(w).stylise(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 40, 24), steps=1, lr=0.1)
