"""CPU: training the backbone's last stage -- the model's ``set_train_backbone`` interface, ``trainable_parameters``, the folded-to-raw
chains of an MBConv block, and the yardstick tests/detector_backbone_ref.py against detector_ref.eager_forward and finite
differences."""
import pytest
import torch

from stlpose_amd import efficientdet as E
from stlpose_amd.detector_train import dw_fold_chain, fold_chain, head_parameters, trainable_parameters
from tests import detector16_ref as R16, detector_backbone_ref as KR, detector_ref as R

BLOCK_PARAMS = ("_expand_conv.conv.weight", "_bn0.weight", "_bn0.bias", "_depthwise_conv.conv.weight", "_bn1.weight", "_bn1.bias",
                "_se_reduce.conv.weight", "_se_reduce.conv.bias", "_se_expand.conv.weight", "_se_expand.conv.bias",
                "_project_conv.conv.weight", "_bn2.weight", "_bn2.bias")
MODELS = (("d0", 1, 16), ("d3", 2, 26))   # name, blocks of the final stage, blocks


def test_set_train_backbone_bounds_and_hints():
    for name, last, nblocks in MODELS:
        m = E.setup_detector("efficientdet", name)
        assert m.train_backbone == 0 and len(m.backbone_net.model._blocks) == nblocks
        assert m.set_train_backbone(0) is m and m.train_backbone == 0   # 0 needs nothing
        with pytest.raises(ValueError, match=r'set_train_bifpn\("all"\)'):
            m.set_train_backbone(1)
        m.set_train_bifpn(len(m.bifpn) - 1)
        with pytest.raises(ValueError, match=r'set_train_bifpn\("all"\)'):
            m.set_train_backbone(1)
        m.set_train_bifpn("all")
        for k in range(last + 1):
            assert m.set_train_backbone(k) is m and m.train_backbone == k
        with pytest.raises(ValueError, match="5x5 / stride-2 depthwise layers whose backward does not exist yet"):
            m.set_train_backbone(last + 1)
        for k in (-1, True, 1.0, "all", None):
            with pytest.raises(ValueError, match=f"expected 0 .. {last}"):
                m.set_train_backbone(k)
        assert m.train_backbone == last
        for x in (0, 1, len(m.bifpn) - 1):
            with pytest.raises(ValueError, match=r"set_train_backbone\(0\)"):
                m.set_train_bifpn(x)
        assert m.set_train_bifpn("all") is m and m.train_bifpn == len(m.bifpn) and m.train_backbone == last
        assert m.set_train_backbone(0).set_train_bifpn(0).train_bifpn == 0


def test_the_limit_comes_from_the_block_specs():
    for name, last, _ in MODELS:
        m = E.setup_detector("efficientdet", name)
        specs = E.block_specs(m.compound_coef)
        stage = [b for b in specs if b["co"] == specs[-1]["co"]]   # the final stage: the blocks with its width
        assert len(stage) == last == m.final_stage_blocks()
        assert all(b["k"] == 3 and b["s"] == 1 and b["e"] == 6 for b in stage) and specs[-1 - last]["k"] == 5
        assert [b["skip"] for b in stage] == [False, True][:last]


def test_trainable_parameter_names_blocks_first():
    for name, last, nblocks in MODELS:
        m = E.setup_detector("efficientdet", name)
        before = [n for n, _ in trainable_parameters(m)]
        assert before == [n for n, _ in head_parameters(m)]
        m.set_train_bifpn("all")
        cells_heads = [n for n, _ in trainable_parameters(m)]
        assert m.set_train_backbone(0) is m and [n for n, _ in trainable_parameters(m)] == cells_heads   # k = 0: what it is today
        params = {n for n, _ in m.named_parameters()}
        for k in range(1, last + 1):
            m.set_train_backbone(k)
            names = [n for n, _ in trainable_parameters(m)]
            want = [f"{KR.PRE}{i}.{t}" for i in range(nblocks - k, nblocks) for t in BLOCK_PARAMS]
            assert names == want + cells_heads
            order = [n for n in m.state_dict() if n in params and n.startswith(tuple(f"{KR.PRE}{i}." for i in range(nblocks - k, nblocks)))]
            assert want == order, "not the state_dict's order"
            named = dict(m.named_parameters())
            assert all(p is named[n] for n, p in trainable_parameters(m))


def test_f16_with_trainable_blocks_raises_naming_fp32():
    m = E.setup_detector("efficientdet", "d0", compute_dtype="f16").set_train_bifpn("all").set_train_backbone(1)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.detection_loss([torch.zeros(3, 64, 64)], [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}])


def _bn_stats(c, g):
    return (torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64),
            torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.3)


def test_depthwise_fold_chain_is_autograd_through_the_fold():
    g = torch.Generator().manual_seed(5)
    c, eps = 7, 1e-3
    gamma, beta, mean, var = _bn_stats(c, g)
    w = torch.randn(c, 3, 3, generator=g, dtype=torch.float64)
    Gw, Gb = torch.randn(c, 3, 3, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    w_, gamma_, beta_ = (t.clone().requires_grad_(True) for t in (w, gamma, beta))
    s = gamma_ / torch.sqrt(var + eps)
    ((w_ * s[:, None, None] * Gw).sum() + ((beta_ - mean * s) * Gb).sum()).backward()
    dw, dgam, dbeta = dw_fold_chain(w, gamma, mean, var, eps, Gw, Gb)
    for got, want in ((dw, w_.grad), (dgam, gamma_.grad), (dbeta, beta_.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)


def test_fold_chain_without_a_conv_bias_is_autograd_through_the_fold():
    g = torch.Generator().manual_seed(6)
    co, ci, eps = 5, 9, 1e-3
    gamma, beta, mean, var = _bn_stats(co, g)
    W = torch.randn(co, ci, generator=g, dtype=torch.float64)
    GW, Gb = torch.randn(co, ci, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
    W_, gamma_, beta_ = (t.clone().requires_grad_(True) for t in (W, gamma, beta))
    s = gamma_ / torch.sqrt(var + eps)
    ((W_ * s[:, None] * GW).sum() + ((beta_ - mean * s) * Gb).sum()).backward()
    dW, db, dgam, dbeta = fold_chain(W, None, gamma, mean, var, eps, GW, Gb)
    assert db is None
    for got, want in ((dW, W_.grad), (dgam, gamma_.grad), (dbeta, beta_.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    # and with a bias it is what it was
    b = torch.randn(co, generator=g, dtype=torch.float64)
    b_ = b.clone().requires_grad_(True)
    for t in (W_, gamma_, beta_):
        t.grad = None
    s = gamma_ / torch.sqrt(var + eps)
    ((W_ * s[:, None] * GW).sum() + ((b_ * s + beta_ - mean * s) * Gb).sum()).backward()
    for got, want in zip(fold_chain(W, b, gamma, mean, var, eps, GW, Gb), (W_.grad, b_.grad, gamma_.grad, beta_.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)


def test_restated_blocks_reproduce_the_eager_forward(monkeypatch):
    """The yardstick's blocks, run in fp64 from the input eager_forward handed the first of them, give the P5 eager_forward handed
    the first cell to 1e-12 relative (D3: through both blocks, the skip included; every fourth pixel of the 512 canvases)."""
    for name, last, nblocks in MODELS:
        m = E.setup_detector("efficientdet", name)
        cc = m.compound_coef
        sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        x = R16.canvas()[:1, :, ::4, ::4].double().contiguous()
        seen, conv = {}, R._conv

        def recording(sd_, p, x_, *a, **kw):
            seen[p] = x_
            return conv(sd_, p, x_, *a, **kw)
        monkeypatch.setitem(E.FPN_REPEATS, cc, 1)
        monkeypatch.setattr(R, "_conv", recording)
        with torch.no_grad():
            R.eager_forward(sd, cc, 1, x)
            monkeypatch.undo()
            specs = E.block_specs(cc)
            y = seen[f"{KR.PRE}{nblocks - last}._expand_conv"]
            for i in range(nblocks - last, nblocks):
                assert seen[f"{KR.PRE}{i}._expand_conv"].shape == y.shape or i == nblocks - last
                y = KR.block_forward(sd, i, specs[i], y)
            want = seen["bifpn.0.p5_down_channel.0"]
        assert y.shape == want.shape and (y - want).abs().max() <= 1e-12 * want.abs().max()


def _tiny_block(skip):
    """mid 8, se 2, a 3 x 3 map, B 2; ci = co = 4 with the skip."""
    g = torch.Generator().manual_seed(11 + skip)
    ci, mid, se, co = 4, 8, 2, 4 if skip else 6
    spec = dict(ci=ci, co=co, k=3, s=1, e=2, mid=mid, se=se, skip=bool(skip))
    p = f"{KR.PRE}0."
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    sd = {p + "_expand_conv.conv.weight": rn(mid, ci, 1, 1) * 0.5, p + "_depthwise_conv.conv.weight": rn(mid, 1, 3, 3) * 0.4,
          p + "_se_reduce.conv.weight": rn(se, mid, 1, 1) * 0.5, p + "_se_reduce.conv.bias": rn(se) * 0.1,
          p + "_se_expand.conv.weight": rn(mid, se, 1, 1), p + "_se_expand.conv.bias": rn(mid) * 0.1,
          p + "_project_conv.conv.weight": rn(co, mid, 1, 1) * 0.4}
    for bn, c in (("_bn0", mid), ("_bn1", mid), ("_bn2", co)):
        gamma, beta, mean, var = _bn_stats(c, g)
        sd.update({p + bn + ".weight": gamma, p + bn + ".bias": beta * 0.1, p + bn + ".running_mean": mean * 0.1,
                   p + bn + ".running_var": var})
    return spec, sd, rn(2, ci, 3, 3), rn(2, co, 3, 3)


@pytest.mark.parametrize("skip", [0, 1])
def test_every_yardstick_gradient_passes_finite_differences(skip):
    spec, sd, x, probe = _tiny_block(skip)
    names = [k for k in sd if not k.endswith(("running_mean", "running_var"))]
    assert sorted(n[len(KR.PRE) + 2:] for n in names) == sorted(BLOCK_PARAMS)

    def f(x_, *params):
        st = dict(sd)
        st.update(zip(names, params))
        return (KR.block_forward(st, 0, spec, x_) * probe).sum()
    inputs = [x.clone().requires_grad_(True)] + [sd[n].clone().requires_grad_(True) for n in names]
    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-7, rtol=1e-6)
    # the variant with the gate held constant is another function: its SE gradients vanish, its depthwise gradient differs
    st = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    (KR.block_forward(st, 0, spec, x, detach_gate=True) * probe).sum().backward()
    assert st[f"{KR.PRE}0._se_expand.conv.weight"].grad is None and st[f"{KR.PRE}0._se_reduce.conv.bias"].grad is None
    full = dict(zip(names, inputs[1:]))
    f(*inputs).backward()
    dwn = f"{KR.PRE}0._depthwise_conv.conv.weight"
    assert (full[dwn].grad - st[dwn].grad).abs().max() > 1e-3 * full[dwn].grad.abs().max()
    pjn = f"{KR.PRE}0._project_conv.conv.weight"
    assert torch.allclose(full[pjn].grad, st[pjn].grad, rtol=1e-12, atol=1e-14)   # the projection does not see the gate's path


def test_tensor_classes_of_a_block():
    assert [KR.tensor_class(f"{KR.PRE}15.{t}") for t in BLOCK_PARAMS] == [
        "expand", "expand_bn", "expand_bn", "depthwise", "depthwise_bn", "depthwise_bn", "se", "se", "se", "se", "project", "project_bn",
        "project_bn"]
    assert set(KR.CLASSES) == {KR.tensor_class(f"{KR.PRE}25.{t}") for t in BLOCK_PARAMS}
