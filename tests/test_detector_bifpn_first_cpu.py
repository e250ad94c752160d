"""CPU: training the first BiFPN cell -- the yardstick tests/detector_bifpn_first_ref.py against detector_ref.eager_forward, and the
model's ``set_train_bifpn("all")`` interface."""
import pytest
import torch

from stlpose_amd import efficientdet as E
from stlpose_amd.detector_train import head_parameters, trainable_parameters
from tests import detector16_ref as R16, detector_bifpn_first_ref as FR, detector_bifpn_ref as BR, detector_ref as R


def _sd64(m):
    sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def test_restated_first_cell_reproduces_the_eager_forward_exactly(monkeypatch):
    """eager_forward stopped behind the first cell gives that cell's outputs; the yardstick's cell 0, run from the P3 / P4 / P5 that
    eager_forward handed its down-channel convs and routed by its own maps, gives them bit for bit in fp64, and with cells 1 and 2
    restated behind it eager_forward's final levels (every fourth pixel of the 512 canvases, as tests/test_detector_bifpn_cpu.py)."""
    m = E.setup_detector("efficientdet", "d0")
    sd = _sd64(m)
    x = R16.canvas()[:, :, ::4, ::4].double().contiguous()
    seen, conv = {}, R._conv

    def recording(sd_, p, x_, *a, **kw):
        seen[p] = x_
        return conv(sd_, p, x_, *a, **kw)
    with torch.no_grad():
        want, _, _ = R.eager_forward(sd, 0, 1, x)
        monkeypatch.setitem(E.FPN_REPEATS, 0, 1)   # eager_forward reads the repeat count from here
        monkeypatch.setattr(R, "_conv", recording)
        want0, _, _ = R.eager_forward(sd, 0, 1, x)
        monkeypatch.undo()
        p3, p4, p5 = (seen[f"bifpn.0.p{i}_down_channel.0"] for i in (3, 4, 5))
        assert seen["bifpn.0.p5_to_p6.0"] is p5 and seen["bifpn.0.p4_down_channel_2.0"] is p4 and seen["bifpn.0.p5_down_channel_2.0"] is p5
        assert [t.shape[1] for t in (p3, p4, p5)] == list(E.P345_CHANNELS[0])
        o = FR.cell0_forward(sd, p3, p4, p5)
        levels = BR.levels_of(o)
        assert all(torch.equal(a, b) for a, b in zip(levels, want0)) and len(levels) == 5
        assert torch.equal(o["p6"], R._pool(o["t"])) and torch.equal(o["p7"], R._pool(o["p6"]))
        for j in (1, 2):
            levels = BR.levels_of(BR.cell_forward(sd, j, levels))
    assert all(torch.equal(a, b) for a, b in zip(levels, want))


def test_set_train_bifpn_all_and_the_integer_bounds():
    for name, cells in (("d0", 3), ("d3", 6)):
        m = E.setup_detector("efficientdet", name)
        assert len(m.bifpn) == cells and m.train_bifpn == 0
        assert m.set_train_bifpn("all") is m and m.train_bifpn == cells
        for k in (cells, -1, cells + 4, True, 1.0, "ALL", None):   # the first cell does not train by count
            with pytest.raises(ValueError, match="first .* does not train"):
                m.set_train_bifpn(k)
        assert m.train_bifpn == cells
        assert m.set_train_bifpn(cells - 1).train_bifpn == cells - 1 and m.set_train_bifpn(0).train_bifpn == 0
    with pytest.raises(ValueError, match="expected 0 .. 5"):
        m.set_train_bifpn(6)
    with pytest.raises(ValueError, match='"all"'):
        m.set_train_bifpn(6)


def test_trainable_parameter_names_with_all():
    m = E.setup_detector("efficientdet", "d0").set_train_bifpn("all")
    names = [n for n, _ in trainable_parameters(m)]
    heads = [n for n, _ in head_parameters(m)]
    params = {n for n, _ in m.named_parameters()}
    want = [n for n in m.state_dict() if n in params and n.startswith("bifpn.")]   # state_dict order: cell 0 first
    assert names == want + heads
    cell0 = [n for n in names if n.startswith("bifpn.0.")]
    assert names[:len(cell0)] == cell0 and len(cell0) == 8 + 8 * 5 + 24 and len(want) == 3 * (8 + 8 * 5) + 24
    new = [n for n in cell0 if n.split(".")[2] in FR.CONVS]
    assert sorted(new) == sorted(f"bifpn.0.{key}.{tail}" for key in FR.CONVS for tail in ("0.conv.weight", "0.conv.bias", "1.weight", "1.bias"))
    named = dict(m.named_parameters())
    assert all(p is named[n] for n, p in trainable_parameters(m))
    assert not any(n.startswith("backbone_net.") for n in names)


def test_f16_with_all_raises_naming_fp32():
    m = E.setup_detector("efficientdet", "d0", compute_dtype="f16").set_train_bifpn("all")
    with pytest.raises(NotImplementedError, match="fp32"):
        m.detection_loss([torch.zeros(3, 64, 64)], [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}])


def test_tensor_classes_of_the_first_cell():
    assert FR.tensor_class("bifpn.0.p5_to_p6.0.conv.weight") == "first_conv" and FR.tensor_class("bifpn.0.p4_down_channel_2.1.bias") == "first_bn"
    assert FR.tensor_class("bifpn.0.conv6_up.bn.weight") == "bn" and FR.tensor_class("bifpn.0.p6_w1") == "fusion"
