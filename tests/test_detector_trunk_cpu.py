"""CPU: training the whole backbone -- the model's ``set_train_trunk`` interface beside ``set_train_backbone``, ``trainable_parameters``
with the stem and the blocks without an expand layer, the header's new entry points, ``DetectorTrainer``'s ``train_trunk`` key, and the
yardstick tests/detector_trunk_ref.py: its blocks against detector_ref.eager_forward, its depthwise adjoint against fp64 autograd under
explicit TF-same padding at every (k, s)."""
import os

import pytest
import torch

from stlpose_amd import capi, efficientdet as E
from stlpose_amd.detector_train import head_parameters, trainable_parameters
from tests import detector16_ref as R16, detector_ref as R, detector_trunk_ref as UR
from tests.test_detector_backbone_cpu import BLOCK_PARAMS, MODELS

STEM_PARAMS = ("backbone_net.model._conv_stem.conv.weight", "backbone_net.model._bn0.weight", "backbone_net.model._bn0.bias")
NO_EXPAND = {"d0": (0,), "d3": (0, 1)}   # the blocks with e = 1


def test_set_train_trunk_argument_rules():
    for name, last, nblocks in MODELS:
        m = E.setup_detector("efficientdet", name)
        assert m.train_backbone == 0 and m.train_stem is False
        assert m.set_train_trunk(0) is m and m.train_backbone == 0   # 0 needs nothing
        for k in (1, nblocks, "all"):
            with pytest.raises(ValueError, match=r'set_train_bifpn\("all"\)'):
                m.set_train_trunk(k)
        m.set_train_bifpn(len(m.bifpn) - 1)
        with pytest.raises(ValueError, match=r'set_train_bifpn\("all"\)'):
            m.set_train_trunk(1)
        m.set_train_bifpn("all")
        for k in range(nblocks + 1):
            assert m.set_train_trunk(k) is m and m.train_backbone == k and m.train_stem is False
        for k in (-1, True, False, 1.0, nblocks + 1, None, "every"):
            with pytest.raises(ValueError, match=f'expected 0 .. {nblocks} .*"all"'):
                m.set_train_trunk(k)
        assert m.train_backbone == nblocks and m.train_stem is False
        assert m.set_train_trunk("all") is m and m.train_backbone == nblocks and m.train_stem is True
        for x in (0, 1, len(m.bifpn) - 1):
            with pytest.raises(ValueError, match=r"set_train_backbone\(0\)"):
                m.set_train_bifpn(x)
        assert m.set_train_bifpn("all") is m and m.train_stem is True
        # the older setter keeps its limit and its texts, and now names the new one
        with pytest.raises(ValueError, match="5x5 / stride-2 depthwise layers whose backward does not exist yet.*set_train_trunk"):
            m.set_train_backbone(last + 1)
        with pytest.raises(ValueError, match=f"expected 0 .. {last}"):
            m.set_train_backbone("all")
        assert m.train_backbone == nblocks and m.train_stem is True


def test_both_setters_clear_the_stem_at_zero_and_agree_below_the_limit():
    for name, last, nblocks in MODELS:
        m = E.setup_detector("efficientdet", name).set_train_bifpn("all")
        assert m.set_train_trunk("all").set_train_backbone(0).train_stem is False and m.train_backbone == 0
        assert m.set_train_trunk("all").set_train_trunk(0).train_stem is False and m.train_backbone == 0
        assert m.set_train_trunk("all").set_train_trunk(nblocks).train_stem is False and m.train_backbone == nblocks
        assert m.set_train_trunk(0).set_train_bifpn(0).train_bifpn == 0
        m.set_train_bifpn("all")
        for k in range(last + 1):
            a = [n for n, _ in trainable_parameters(m.set_train_trunk(k))]
            va = m._state_version()
            m.set_train_trunk(0)
            b = [n for n, _ in trainable_parameters(m.set_train_backbone(k))]
            assert a == b and m.train_backbone == k and m.train_stem is False and va == m._state_version()
        assert m.set_train_trunk("all").set_train_backbone(last).train_stem is False and m.train_backbone == last


def test_a_change_of_k_drops_the_plans_backward():
    class Plan:
        train = "listed"
    m = E.setup_detector("efficientdet", "d0").set_train_bifpn("all")
    for change in (lambda: m.set_train_trunk(5), lambda: m.set_train_trunk("all"), lambda: m.set_train_trunk(16), lambda: m.set_train_backbone(0)):
        m._plans = {2: Plan()}
        change()
        assert m._plans[2].train is None
    m._plans = {2: Plan()}
    m.set_train_trunk(0)
    assert m._plans[2].train == "listed"   # nothing changed
    m._plans = {}


def test_trainable_parameter_names_stem_first_then_blocks_of_10_or_13():
    for name, last, nblocks in MODELS:
        m = E.setup_detector("efficientdet", name)
        m.set_train_bifpn("all")
        cells_heads = [n for n, _ in trainable_parameters(m)]
        assert cells_heads[-len(head_parameters(m)):] == [n for n, _ in head_parameters(m)]
        params = {n for n, _ in m.named_parameters()}
        named = dict(m.named_parameters())

        def block_names(i):
            return [f"{UR.PRE}{i}.{t}" for t in (BLOCK_PARAMS[3:] if i in NO_EXPAND[name] else BLOCK_PARAMS)]
        for k in (last + 1, nblocks // 2, nblocks - 1, nblocks, "all"):
            m.set_train_trunk(k)
            kk = nblocks if k == "all" else k
            names = [n for n, _ in trainable_parameters(m)]
            want = (list(STEM_PARAMS) if k == "all" else []) + [n for i in range(nblocks - kk, nblocks) for n in block_names(i)]
            assert names == want + cells_heads
            order = [n for n in m.state_dict() if n in params and n in set(want)]
            assert want == order, "not the state_dict's order"
            assert all(p is named[n] for n, p in trainable_parameters(m))
        every = [n for n, _ in trainable_parameters(m)]
        assert sorted(every) == sorted(params), "\"all\" with every cell is every parameter of the model"
        per_block = [sum(n.startswith(f"{UR.PRE}{i}.") for n in every) for i in range(nblocks)]
        assert per_block == [10 if i in NO_EXPAND[name] else 13 for i in range(nblocks)]
        assert every[:3] == list(STEM_PARAMS)
        assert [b["e"] == 1 for b in E.block_specs(m.compound_coef)] == [i in NO_EXPAND[name] for i in range(nblocks)]


def test_state_version_puts_the_stem_with_the_blocks():
    m = E.setup_detector("efficientdet", "d0").set_train_bifpn("all")
    net = m.backbone_net.model
    stem = {t.data_ptr() for t in list(net._conv_stem.parameters()) + list(net._bn0.parameters()) + list(net._bn0.buffers())}
    ptrs = lambda group: {p for p, _ in group}  # noqa: E731
    v = m.set_train_trunk(16)._state_version()
    assert stem <= ptrs(v[0]) and not stem & ptrs(v[1])
    v = m.set_train_trunk("all")._state_version()
    assert stem <= ptrs(v[1]) and not stem & ptrs(v[0])
    assert all(t.data_ptr() in ptrs(v[1]) for t in net._blocks.parameters())


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(capi.INCLUDE, "stlpose_hip_det_mbconv.h")).read()
    for fn in ("int stl_det_dwconv_bwd_data_ks(const float* dy, const float* w, const float* z, float* dx, int B, int H, int W, int C, int k, int s,",
               "int stl_det_dwconv_bwd_weight_ks(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, int C, int k, int s,",
               "int stl_det_dwconv_bwd_ks_parts(int64_t npix);",
               "int stl_det_stem_bwd(const float* x, const float* w, const float* bias, const float* dy, float* partial, float* dw, float* db, int B,",
               "int stl_det_stem_bwd_parts(int64_t npix);"):
        assert fn in text, fn
    names = set(capi.DET_MBCONV.signatures)   # the ctypes binding is derived from the header
    assert {"stl_det_dwconv_bwd_data_ks", "stl_det_dwconv_bwd_weight_ks", "stl_det_dwconv_bwd_ks_parts", "stl_det_stem_bwd",
            "stl_det_stem_bwd_parts", "stl_det_mbconv_gate_bwd"} <= names


def test_f16_with_a_trainable_trunk_raises_naming_fp32():
    for k in (3, "all"):
        m = E.setup_detector("efficientdet", "d0", compute_dtype="f16").set_train_bifpn("all").set_train_trunk(k)
        with pytest.raises(NotImplementedError, match="fp32"):
            m.detection_loss([torch.zeros(3, 64, 64)], [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}])


def test_detector_trainer_takes_train_trunk_and_refuses_both_keys(tmp_path):
    from stlpose_amd import detector_trainer
    from tests.test_det_batch_cpu import _StubLoader, _exp_data
    gt = {"annotations": [dict(image_id=1, category_id=1, bbox=[0, 0, 5, 5], area=25.0, iscrowd=0, id=1)], "categories": [{"id": 1}]}

    def trainer(model, **training):
        return detector_trainer.DetectorTrainer(str(tmp_path), _exp_data(**training), model, _StubLoader([1.0]), _StubLoader([1.0]), gt,
                                                device="cpu")
    m = E.setup_detector("efficientdet", "d0")
    with pytest.raises(ValueError, match="both train_backbone and train_trunk"):
        trainer(m, train_bifpn="all", train_backbone=1, train_trunk=4)
    assert m.train_backbone == 0 and m.train_bifpn == 0
    for k, blocks, stem in ((4, 4, False), ("all", 16, True), (16, 16, False), (0, 0, False)):
        t = trainer(m, train_bifpn="all", train_trunk=k)
        assert (m.train_bifpn, m.train_backbone, m.train_stem) == (3, blocks, stem)
        optimised = {id(q) for group in t.optimizer.param_groups for q in group["params"]}
        assert optimised == {id(q) for _, q in trainable_parameters(m)}
    trainer(m, train_bifpn="all", train_trunk="all")
    trainer(m, train_bifpn="all", train_backbone=1)   # the older key alone still works, and clears the stem
    assert (m.train_backbone, m.train_stem) == (1, False)
    trainer(m, train_bifpn="all", train_trunk="all")
    trainer(m, train_bifpn=0)                          # neither key: nothing of the backbone trains
    assert (m.train_bifpn, m.train_backbone, m.train_stem) == (0, 0, False)


def test_restated_blocks_and_stem_reproduce_the_eager_forward(monkeypatch):
    """The yardstick's stem and every block of D0, chained in fp64 from the canvas, give the P3 / P4 / P5 eager_forward handed the first
    cell to 1e-12 relative (every fourth pixel of a 512 canvas: 128 x 128, whose stride-2 maps have even and odd sizes)."""
    m = E.setup_detector("efficientdet", "d0")
    sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = R16.canvas()[:1, :, ::4, ::4][:, :, :127, :126].double().contiguous()
    seen, conv = {}, R._conv

    def recording(sd_, p, x_, *a, **kw):
        seen[p] = x_
        return conv(sd_, p, x_, *a, **kw)
    monkeypatch.setitem(E.FPN_REPEATS, 0, 1)
    monkeypatch.setattr(R, "_conv", recording)
    with torch.no_grad():
        R.eager_forward(sd, 0, 1, x)
        monkeypatch.undo()
        specs = E.block_specs(0)
        y, maps = UR.stem_forward(sd, x), {}
        for i, b in enumerate(specs):
            maps[i] = y
            y = UR.block_forward(sd, i, b, y)
    for got, key in ((maps[5], "bifpn.0.p3_down_channel.0"), (maps[11], "bifpn.0.p4_down_channel.0"), (y, "bifpn.0.p5_down_channel.0")):
        want = seen[key]
        assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max(), key


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_adjoint_is_autograd_under_same_padding(k, s):
    """The gather the kernels implement, against F.conv2d's autograd under explicit TF-same padding, on maps of both parities."""
    g = torch.Generator().manual_seed(10 * k + s)
    for H, W in ((7, 6), (6, 7), (1, 1), (2, 3)):
        pads = (UR.same_pad_before(H, k, s), UR.same_pad_before(W, k, s))
        if s == 2:
            assert pads == tuple({(3, 0): 0, (3, 1): 1, (5, 0): 1, (5, 1): 2}[k, n % 2] if n > 1 else (k - 1) // 2 for n in (H, W))
        else:
            assert pads == ((k - 1) // 2,) * 2
        Ho, Wo = -(-H // s), -(-W // s)
        x, w = torch.randn(2, 4, H, W, generator=g, dtype=torch.float64), torch.randn(4, k, k, generator=g, dtype=torch.float64)
        dy = torch.randn(2, 4, Ho, Wo, generator=g, dtype=torch.float64)
        dx, _ = UR.dw_autograd(x, w, dy, k, s)
        got = UR.dw_adjoint(dy, w, H, W, k, s)
        assert (got - dx).abs().max() <= 1e-13 * max(1.0, dx.abs().max().item()), (H, W)
        z = torch.randn(2, 4, H, W, generator=g, dtype=torch.float64)
        sg = torch.sigmoid(z)
        dxz, _ = UR.dw_autograd(x, w, dy, k, s, z)
        assert torch.allclose(dxz, dx * (sg * (1 + z * (1 - sg))), rtol=1e-12, atol=1e-14)


def test_tensor_classes_of_the_trunk():
    assert [UR.tensor_class(n) for n in STEM_PARAMS] == ["stem", "stem_bn", "stem_bn"]
    assert UR.tensor_class(f"{UR.PRE}0._bn0.weight") == "expand_bn" and UR.tensor_class(f"{UR.PRE}3._depthwise_conv.conv.weight") == "depthwise"
