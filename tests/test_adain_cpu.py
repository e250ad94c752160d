"""CPU: host side of the AdaIN stylizer (stlpose_amd/adain.py) and of the Styled-COCO producer (stlpose_amd/styled_coco.py):
weight-file layouts, the folded input conv, the one-affine form of AdaIN + alpha, argument errors, and the producer's paths,
style draw and batching with a stub stylizer.  Checked against tests/adain_ref.py.  PARITY UNPINNED (no reference counterpart)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from stlpose_amd import AdaINStylizer, create_styled_dataset
from stlpose_amd.adain import DECODER_LAYOUT, ENCODER_LAYOUT, affine_coefficients, conv_macs, fold_input_conv
from stlpose_amd.perceptual_offline import dict_filename
from stlpose_amd.styled_coco import styled_dir

from tests import adain_ref as R

ENC, DEC = R.synth()


def test_layout_matches_the_published_sequentials():
    assert len(ENC) == 31 and len(DEC) == 29
    assert [i for i, m in enumerate(ENC) if isinstance(m, nn.Conv2d)] == [0] + [r[0] for r in ENCODER_LAYOUT]
    assert [i for i, m in enumerate(DEC) if isinstance(m, nn.Conv2d)] == [r[0] for r in DECODER_LAYOUT]
    assert [i for i, m in enumerate(ENC) if isinstance(m, nn.MaxPool2d)] == [7, 14, 27]
    assert [i for i, m in enumerate(DEC) if isinstance(m, nn.Upsample)] == [3, 16, 23]
    for seq, layout in ((ENC, ENCODER_LAYOUT), (DEC, DECODER_LAYOUT)):
        for idx, ci, co, op in layout:
            assert tuple(seq[idx].weight.shape) == (co, ci, 3, 3)
            before = seq[idx - 2] if idx >= 2 else None     # what sits in front of the conv's reflection pad
            assert (op == "pool") == isinstance(before, nn.MaxPool2d) and (op == "up") == isinstance(before, nn.Upsample)


def test_weight_files_load_and_state_dict_round_trips():
    m = AdaINStylizer(ENC.state_dict(), DEC.state_dict())
    sd = m.state_dict()
    assert set(sd) == {f"encoder.{k}" for k in ENC.state_dict()} | {f"decoder.{k}" for k in DEC.state_dict()}
    for k, v in ENC.state_dict().items():
        assert torch.equal(sd[f"encoder.{k}"], v)
    for k, v in DEC.state_dict().items():
        assert torch.equal(sd[f"decoder.{k}"], v)
    assert not any(p.requires_grad for p in m.parameters())
    m2 = AdaINStylizer()
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))
    m3 = AdaINStylizer(compute_dtype="bf16")
    m3.load_encoder_weights(ENC.state_dict())
    m3.load_decoder_weights(DEC.state_dict())
    assert torch.equal(m3.state_dict()["decoder.28.bias"], DEC.state_dict()["28.bias"])


def test_whole_vgg19_file_loads_and_missing_key_is_named():
    sd = dict(ENC.state_dict())
    sd["32.weight"], sd["32.bias"] = torch.zeros(512, 512, 3, 3), torch.zeros(512)   # relu4_2 .. of the full VGG19 file
    sd["51.weight"] = torch.zeros(512, 512, 3, 3)
    m = AdaINStylizer()
    m.load_encoder_weights(sd)
    assert torch.equal(m.state_dict()["encoder.29.weight"], sd["29.weight"]) and "encoder.32.weight" not in m.state_dict()
    short = {k: v for k, v in ENC.state_dict().items() if k != "16.bias"}
    with pytest.raises(KeyError, match="16.bias"):
        AdaINStylizer().load_encoder_weights(short)
    with pytest.raises(KeyError, match="28.weight"):
        AdaINStylizer(decoder_state_dict={k: v for k, v in DEC.state_dict().items() if k != "28.weight"})
    with pytest.raises(ValueError):
        AdaINStylizer(compute_dtype="fp16")


def test_folded_conv1_1_equals_conv0_pad_conv1_1():
    """Within 1e-5 of the output's maximum (the fold is exact in exact arithmetic; measured 3e-7)."""
    m = AdaINStylizer(ENC.state_dict(), DEC.state_dict())
    w, b = m.folded_conv1_1()
    assert tuple(w.shape) == (64, 3, 3, 3) and tuple(b.shape) == (64,)
    x = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(1))
    ref = ENC[2](ENC[1](ENC[0](x)))
    got = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    err = R.rel_err(got, ref)
    print(f"folded conv1_1: {err:.2e}")
    assert err < 1e-5
    w2, b2 = fold_input_conv(ENC[0].weight, ENC[0].bias, ENC[2].weight, ENC[2].bias)
    assert torch.equal(w, w2) and torch.equal(b, b2)


@pytest.mark.parametrize("alpha", [1.0, 0.6, 0.0])
@pytest.mark.parametrize("mode", ["one", "per_image", "weights"])
def test_affine_is_the_two_step_form(mode, alpha):
    """f * scale + offset against adain_ref's normalise / re-style / blend, in fp64."""
    g = torch.Generator().manual_seed(2)
    B, C = 3, 16
    fc = torch.randn(B, C, 6, 5, generator=g, dtype=torch.float64).clamp_min(0.0) * 3 + 1
    fc[:, 2] = 0.0                                              # a dead channel: sigma_c = sqrt(eps)
    S = {"one": 1, "per_image": B, "weights": 4}[mode]
    fs = torch.randn(S, C, 4, 7, generator=g, dtype=torch.float64) * 2 + 0.5
    w = torch.tensor([[0.1, 0.2, 0.3, 0.4], [1.0, 0.0, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25]], dtype=torch.float64) if mode == "weights" else None
    ms, ss = R.mean_sigma(fs)
    if w is not None:
        msb, ssb = (w @ ms.flatten(1)).view(B, C, 1, 1), (w @ ss.flatten(1)).view(B, C, 1, 1)
    else:
        msb, ssb = ms.expand(B, -1, -1, -1), ss.expand(B, -1, -1, -1)
    ref = R.adain(fc, msb, ssb, alpha)
    flat = fc.reshape(B, C, -1)
    scale, offset = affine_coefficients(flat.mean(2), flat.var(2), ms.flatten(1), ss.flatten(1), alpha, w)
    got = fc * scale.view(B, C, 1, 1) + offset.view(B, C, 1, 1)
    assert scale.dtype == torch.float64
    assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    if alpha == 0.0:
        assert torch.all(scale == 1) and torch.all(offset == 0)


def test_affine_rejects_bad_style_counts_and_weights():
    z = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="2 styles for 3"):
        affine_coefficients(z, z + 1, torch.zeros(2, 8), torch.ones(2, 8), 1.0)
    with pytest.raises(ValueError, match="sum to 1"):
        affine_coefficients(z, z + 1, torch.zeros(2, 8), torch.ones(2, 8), 1.0, torch.ones(3, 2))
    with pytest.raises(ValueError):
        affine_coefficients(z, z + 1, torch.zeros(2, 8), torch.ones(2, 8), 1.0, torch.full((2, 2), 0.5))


def test_argument_errors():
    m = AdaINStylizer(ENC.state_dict(), DEC.state_dict())
    ok = torch.rand(1, 3, 32, 32)
    for bad in [(1, 3, 36, 32), (1, 3, 32, 8), (1, 3, 20, 64)]:
        with pytest.raises(ValueError, match=f"{bad[2]}x{bad[3]}"):
            m.stylise(torch.rand(bad), ok)
        with pytest.raises(ValueError, match=f"{bad[2]}x{bad[3]}"):
            m.prepare_style(torch.rand(bad))
    for alpha in (-0.1, 1.5):
        with pytest.raises(ValueError, match="alpha"):
            m.stylise(ok, ok, alpha=alpha)
    with pytest.raises(ValueError):
        m.stylise(torch.rand(1, 1, 32, 32), ok)
    with pytest.raises(RuntimeError, match="no CPU path"):     # as the other modules
        m.stylise(ok, ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.prepare_style(ok)


def test_conv_macs_counts_the_ring():
    true, padded = conv_macs(1, 64, 64, False), conv_macs(1, 64, 64, True)
    seq = nn.Sequential(*list(ENC)[1:], *list(DEC))     # true sizes: conv1_1 .. the last decoder conv
    macs, x = 0, torch.zeros(1, 3, 64, 64)
    for mod in seq:
        x = mod(x)
        if isinstance(mod, nn.Conv2d):
            macs += x.shape[2] * x.shape[3] * mod.weight.numel()
    assert true == macs
    assert true < padded < 1.3 * true


class _Stub:
    """Stands in for AdaINStylizer: records its calls, 'stylises' by inverting the image."""

    def __init__(self):
        self.batches, self.prepared = [], 0

    def prepare_style(self, style):
        self.prepared += 1
        return torch.full((1, 4), float(self.prepared - 1)), torch.ones(1, 4)

    def stylise(self, content, style, alpha=1.0, clamp=True):
        self.batches.append((tuple(content.shape), style[0][:, 0].tolist(), alpha, clamp))
        return 1.0 - content


def _images():
    g = torch.Generator().manual_seed(0)
    sizes = [(32, 48)] * 3 + [(40, 24)] * 2 + [(32, 48)]
    out = []
    for i, (h, w) in enumerate(sizes):
        if i % 2:
            out.append((f"{i:03d}.jpg", torch.rand(3, h, w, generator=g)))
        else:
            out.append((f"{i:03d}.jpg", (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()))
    return out


def test_producer_paths_draw_and_batching(tmp_path):
    imgs, styles = _images(), [torch.rand(3, 16, 16) for _ in range(5)]
    stub, rec = _Stub(), []
    man = create_styled_dataset(stub, imgs, styles, str(tmp_path), "vases", 0.5, seed=1, batch=2, split="val",
                                writer=lambda p, a: rec.append((p, a)), device="cpu")
    root = os.path.join(str(tmp_path), "images_style_vases_alpha_0.5", "val")
    assert styled_dir(str(tmp_path), "vases", 0.5, "val") == root
    assert stub.prepared == 5                                  # each style prepared once
    # batches: equal consecutive sizes, at most `batch`: [0, 1], [2], [3, 4], [5]
    assert [b[0] for b in stub.batches] == [(2, 3, 32, 48), (1, 3, 32, 48), (2, 3, 40, 24), (1, 3, 32, 48)]
    assert all(b[2] == 0.5 and b[3] is True for b in stub.batches)
    assert [p for p, _ in rec] == [os.path.join(root, n) for n, _ in imgs] and list(man) == [n for n, _ in imgs]
    drawn = [man[n]["style"] for n, _ in imgs]
    import random
    rng = random.Random(1)
    assert drawn == [rng.randrange(5) for _ in imgs]           # one draw per image, in iteration order
    assert [k for b in stub.batches for k in b[1]] == [float(k) for k in drawn]   # the batch got its images' styles
    assert all(man[n]["path"] == os.path.join(root, n) for n, _ in imgs)
    for (name, src), (_, arr) in zip(imgs, rec):
        assert arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[2] == 3
        if isinstance(src, np.ndarray):
            assert np.array_equal(arr, 255 - src)              # the stub's inversion, back in uint8 HWC
    # same seed -> same manifest; another seed -> another draw
    again = create_styled_dataset(_Stub(), imgs, styles, str(tmp_path), "vases", 0.5, seed=1, batch=4, split="val",
                                  writer=lambda p, a: None, device="cpu")
    assert again == man
    other = create_styled_dataset(_Stub(), imgs, styles, str(tmp_path), "vases", 0.5, seed=2, split="val", writer=lambda p, a: None,
                                  device="cpu")
    assert [v["style"] for v in other.values()] != drawn
    assert not os.path.exists(root)                            # the recording writer touched no file


def test_producer_json_name_and_argument_errors(tmp_path, monkeypatch):
    imgs, styles = _images()[:2], [torch.rand(3, 16, 16)]
    calls = {}

    def fake_offline(pairs, vgg, dict_path, alpha, styles_tag, device="cuda"):
        calls["names"] = [(n, tuple(s.shape), tuple(o.shape)) for n, s, o in pairs]
        calls["file"] = os.path.join(dict_path, dict_filename(alpha, styles_tag))
        return {}

    import stlpose_amd.styled_coco as sc
    monkeypatch.setattr(sc, "create_offline_perceptual_loss", fake_offline)
    create_styled_dataset(_Stub(), imgs, styles, str(tmp_path), 3, 1.0, vgg=object(), dict_path=str(tmp_path / "d"),
                          writer=lambda p, a: None, device="cpu")
    assert calls["file"] == os.path.join(str(tmp_path / "d"), "perceptual_loss_dict_alpha_1.0_styles_3.json")
    assert calls["names"] == [(n, (3, 32, 48), (3, 32, 48)) for n, _ in imgs]
    with pytest.raises(ValueError, match="go together"):
        create_styled_dataset(_Stub(), imgs, styles, str(tmp_path), 3, 1.0, vgg=object(), writer=lambda p, a: None, device="cpu")
    with pytest.raises(ValueError, match="no style"):
        create_styled_dataset(_Stub(), imgs, [], str(tmp_path), 3, 1.0, writer=lambda p, a: None, device="cpu")
    with pytest.raises(ValueError, match="at least 16"):
        create_styled_dataset(_Stub(), [("tiny.png", torch.rand(3, 8, 32))], styles, str(tmp_path), 3, 1.0, writer=lambda p, a: None,
                              device="cpu")
