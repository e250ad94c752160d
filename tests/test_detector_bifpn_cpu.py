"""CPU: the yardstick of the BiFPN fine-tuning tests (tests/detector_bifpn_ref.py) against detector_ref.eager_forward, the
fusion-weight Jacobian of detector_train against autograd, and the model's train_bifpn interface."""
import pytest
import torch
import torch.nn.functional as F

from stlpose_amd import efficientdet as E
from stlpose_amd.detector_train import fusion_weight_grads, head_parameters, trainable_parameters
from tests import detector16_ref as R16, detector_bifpn_ref as BR, detector_ref as R


def _sd64(m):
    sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def test_restated_cells_reproduce_the_eager_forward_exactly(monkeypatch):
    """eager_forward stopped behind the first cell gives that cell's outputs; cells 1 and 2 restated behind them give
    eager_forward's final levels bit for bit, in fp64 on the test images (every fourth pixel of their 512 canvases: the fp64
    network runs twice on the host, and the restatement does not depend on the size; P3 is 16 x 16 and P7 one pixel)."""
    m = E.setup_detector("efficientdet", "d0")
    sd = _sd64(m)
    x = R16.canvas()[:, :, ::4, ::4].double().contiguous()
    with torch.no_grad():
        want, _, _ = R.eager_forward(sd, 0, 1, x)
        monkeypatch.setitem(E.FPN_REPEATS, 0, 1)   # eager_forward reads the repeat count from here
        levels, _, _ = R.eager_forward(sd, 0, 1, x)
        monkeypatch.undo()
        levels = list(levels)
        for j in (1, 2):
            levels = BR.levels_of(BR.cell_forward(sd, j, levels))
    assert all(torch.equal(a, b) for a, b in zip(levels, want)) and len(levels) == 5


@pytest.mark.parametrize("hw", [(5, 5), (6, 6), (8, 8), (7, 4)])
def test_routed_pool_equals_max_pool_when_routed_from_its_own_input(hw):
    g = torch.Generator().manual_seed(hw[0] * 10 + hw[1])
    x = torch.randn(2, 3, *hw, generator=g)
    x[0, 0] = -x[0, 0].abs() - 0.1   # a channel whose border windows the padding wins
    x[1, 1, 1, 1] = x[1, 1, 1, 2] = 9.0   # an exact tie
    want = F.max_pool2d(R._same(x, 3, 2), 3, 2)
    assert torch.equal(BR.routed_pool(x), want) and torch.equal(BR.routed_pool(x.double(), x), want.double())
    # routed from another map it follows that map's winners, not its own
    other = torch.randn(2, 3, *hw, generator=g)
    y = BR.routed_pool(x.double(), other)
    _, idx = F.max_pool2d(R._same(other, 3, 2), 3, 2, return_indices=True)
    assert torch.equal(y, R._same(x.double(), 3, 2).flatten(2).gather(2, idx.flatten(2)).view(idx.shape))


@pytest.mark.parametrize("p", [[0.7, 1.3], [0.4, 1.1, 0.9], [1.2, -0.3, 0.8], [0.0, 0.6]])
def test_fusion_weight_jacobian_matches_autograd(p):
    p = torch.tensor(p, dtype=torch.float64)
    g = torch.Generator().manual_seed(len(p))
    dwhat = torch.randn(len(p), generator=g, dtype=torch.float64)
    q = p.clone().requires_grad_(True)
    (BR.fusion_weights(q) * dwhat).sum().backward()
    got = fusion_weight_grads(p, dwhat)
    assert torch.allclose(got, q.grad, rtol=1e-13, atol=1e-15), (got, q.grad)
    assert (got[p <= 0] == 0).all()


def test_set_train_bifpn_bounds():
    m = E.setup_detector("efficientdet", "d0")
    assert m.train_bifpn == 0 and len(m.bifpn) == 3
    for k in (3, -1, 7):
        with pytest.raises(ValueError, match="first .* does not train"):
            m.set_train_bifpn(k)
    assert m.train_bifpn == 0
    assert m.set_train_bifpn(2) is m and m.train_bifpn == 2
    m3 = E.setup_detector("efficientdet", "d3")
    m3.set_train_bifpn(5)
    with pytest.raises(ValueError, match="expected 0 .. 5"):
        m3.set_train_bifpn(6)


def test_trainable_parameter_names():
    m = E.setup_detector("efficientdet", "d0")
    heads = [n for n, _ in head_parameters(m)]
    keys = list(m.state_dict())
    params = {n for n, _ in m.named_parameters()}
    for k in (0, 1, 2):
        m.set_train_bifpn(k)
        names = [n for n, _ in trainable_parameters(m)]
        cells = tuple(f"bifpn.{j}." for j in range(3 - k, 3))
        want = [n for n in keys if n in params and k and n.startswith(cells)]   # state_dict order
        assert names == want + heads
        assert len(want) == k * (8 + 8 * 5)   # per cell eight fusion weights and eight nodes of dw, pw weight, pw bias, BN weight, BN bias
        named = dict(m.named_parameters())
        assert all(p is named[n] for n, p in trainable_parameters(m))
    assert [n for n, _ in head_parameters(m)] == heads
