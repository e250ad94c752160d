"""CPU: the yardstick of the VGG layer tests (tests/vgg_layers_ref.py) is the pinned oracle, its bounds reject the faults that the
loss scalars let through, and the image shapes of the GPU tests have the properties the comparison rests on."""
import pytest
import torch

from oracle import vgg_ref
from tests import vgg_layers_ref as L


def chain(img_n, weights, rows, dtype, bf16_weights=False):
    """Every layer fed the previous layer's result in `dtype` -> the list of layer outputs."""
    out, x = [], img_n
    for idx, pool in rows:
        x = L.layer(x, weights[f"features.{idx}.weight"], weights[f"features.{idx}.bias"], pool, dtype, bf16_weights)
        out.append(x)
    return out


@pytest.fixture(scope="module")
def vgg16_44x36():
    """fp64 and fp32 chains of the 44 x 36 case (input and target as one batch) on VGG16."""
    w = vgg_ref.synth_vgg_weights()
    x = torch.cat(L.case_images("vgg16", "44x36"), 0)
    return w, chain(L.normalise(x, torch.float64), w, L.VGG16_ROWS, torch.float64), chain(L.normalise(x, torch.float32), w, L.VGG16_ROWS, torch.float32)


@pytest.fixture(scope="module")
def vgg19_44x36():
    w = vgg_ref.synth_vgg19_weights()
    x = torch.cat(L.case_images("vgg19", "2x44x36"), 0)
    return w, chain(L.normalise(x, torch.float64), w, L.VGG19_ROWS, torch.float64), chain(L.normalise(x, torch.float32), w, L.VGG19_ROWS, torch.float32)


# ------------------------------------------------------------------------------------------------ chaining == the pinned oracle
def test_chained_layers_are_the_oracle_vgg16(vgg16_44x36):
    w, _, y32 = vgg16_44x36
    x = L.normalise(torch.cat(L.case_images("vgg16", "44x36"), 0), torch.float32)
    mean = torch.tensor(vgg_ref.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(vgg_ref.IMAGENET_STD).view(1, 3, 1, 1)
    assert torch.equal(x, (torch.cat(L.case_images("vgg16", "44x36"), 0) - mean) / std)   # vgg_perceptual_loss's own line
    feats = vgg_ref.vgg_features(x, w)
    assert len(L.VGG16_ROWS) == 10 and len(feats) == len(L.VGG16_SLICE_END)
    for f, i in zip(feats, L.VGG16_SLICE_END):
        assert torch.equal(f, y32[i]), i


def test_chained_layers_are_the_oracle_vgg19(vgg19_44x36):
    w, _, y32 = vgg19_44x36
    taps = vgg_ref.vgg19_taps(L.normalise(torch.cat(L.case_images("vgg19", "2x44x36"), 0), torch.float32), w)
    assert len(taps) == len(y32) == 13
    for i, (a, b) in enumerate(zip(taps, y32)):
        assert torch.equal(a, b), i
    for i in vgg_ref.VGG19_STYLE_TAPS:
        assert torch.equal(vgg_ref.gram(y32[i]), L.gram(y32[i], torch.float32))


# ------------------------------------------------------------------------------------------------ the bounds catch what the scalars miss
def rejected(fn, *args) -> bool:
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def faults(y, refault_bias):
    """The seeded faults of one layer's fp32 result y [B, C, H, W]."""
    dup = y.clone()
    dup[:, -8:] = y[:, -16:-8]
    corner = y.clone()
    corner[:, :, -1, -1] = 0
    col = y.clone()
    col[..., -1] = y[..., -2]
    return {"last 8 biases zeroed": refault_bias(), "last 8 channels from the neighbouring group": dup,
            "corner pixel zeroed": corner, "last column copied from its neighbour": col}


@pytest.mark.parametrize("pos", [0, 1, 5, 8, 9])   # features.0, .2, .12, .19, .21
def test_bounds_reject_seeded_layer_faults(vgg16_44x36, pos):
    w, c64, c32 = vgg16_44x36
    idx, pool = L.VGG16_ROWS[pos]
    wt, bs = w[f"features.{idx}.weight"], w[f"features.{idx}.bias"]
    xin = L.normalise(torch.cat(L.case_images("vgg16", "44x36"), 0), torch.float32) if pos == 0 else c32[pos - 1]
    y64, y32 = L.layer(xin, wt, bs, pool, torch.float64), L.layer(xin, wt, bs, pool, torch.float32)
    assert torch.equal(y32, c32[pos])
    # the unfaulted tensor passes both
    L.hold("clean", y32, y64, y32)
    L.hold16("clean bf16", y32.bfloat16(), y64, y32)

    def no_tail_bias():
        b = bs.clone()
        b[-8:] = 0
        return L.layer(xin, wt, b, pool, torch.float32)
    for name, bad in faults(y32, no_tail_bias).items():
        assert not torch.equal(bad, y32), name
        assert rejected(L.hold, name, bad, y64, y32, L.MARGIN_CONV32), name
        assert rejected(L.hold16, name, bad.bfloat16(), y64, y32), name
    # bf16 plan: the yardstick with bf16-rounded weights accepts the bf16 result of those weights, rejects the faults alike
    z64, z32 = L.layer(xin, wt, bs, pool, torch.float64, True), L.layer(xin, wt, bs, pool, torch.float32, True)
    L.hold16("clean bf16 weights", z32.bfloat16(), z64, z32)
    for name, bad in faults(z32, lambda: L.layer(xin, wt, torch.cat([bs[:-8], torch.zeros(8)]), pool, torch.float32, True)).items():
        assert rejected(L.hold16, name, bad.bfloat16(), z64, z32), name


@pytest.mark.parametrize("tap", [0, 2, 4])   # relu1_1, relu2_1, relu3_1
def test_bounds_reject_gram_without_last_pixel_row(vgg19_44x36, tap):
    _, _, c32 = vgg19_44x36
    f = c32[tap]
    g64, g32 = L.gram(f, torch.float64), L.gram(f, torch.float32)
    L.hold("clean gram", g32, g64, g32)
    L.hold("clean gram symmetry", g32.transpose(1, 2), g64, g32)
    b, c, h, w = f.shape
    short = L.gram(f[:, :, :-1], torch.float32) * ((h - 1) / h)   # the sum without the last row, over the full C H W
    assert rejected(L.hold, "gram without its last pixel row", short, g64, g32)


def test_first_link_in_bf16_is_two_links():
    """Why the bf16 GPU test checks conv1_1 from the STORED patches, and the patches against the image: an implementation that
    is exact apart from storing the normalised patches in bf16 (one rounding, as the plan's 16-bit activations are stored) does
    not meet the elementwise bound against the un-rounded image -- that bound allows one rounding of the OUTPUT only.  From
    its own stored input it does."""
    w = vgg_ref.synth_vgg_weights()
    wt, bs = w["features.0.weight"], w["features.0.bias"]
    x = torch.cat(L.case_images("vgg16", "44x36"), 0)
    x64, x32 = L.normalise(x, torch.float64), L.normalise(x, torch.float32)
    stored = x32.bfloat16()
    L.hold16("patches", stored, x64, x32)
    y64, y32 = L.layer(x64, wt, bs, False, torch.float64, True), L.layer(x32, wt, bs, False, torch.float32, True)
    exact16 = L.layer(stored, wt, bs, False, torch.float64, True).bfloat16()
    assert rejected(L.hold16, "conv1_1 from the image", exact16, y64, y32)
    L.hold16("conv1_1 from the stored patches", exact16, L.layer(stored, wt, bs, False, torch.float64, True),
             L.layer(stored, wt, bs, False, torch.float32, True))


# ------------------------------------------------------------------------------------------------ what the GPU comparison rests on
def pool_inputs(H, W, rows):
    out, h, w = [], H, W
    for _, pool in rows:
        if pool:
            out.append((h, w))
            h, w = h // 2, w // 2
    return out, (h, w)


def test_shapes_have_odd_pool_inputs_and_minimum_maps():
    p16 = {n: pool_inputs(224 if c["resize"] else c["H"], 224 if c["resize"] else c["W"], L.VGG16_ROWS) for n, c in L.VGG16_CASES.items()}
    p19 = {n: pool_inputs(c["H"], c["W"], L.VGG19_ROWS) for n, c in L.VGG19_CASES.items()}
    for table in (p16, p19):
        assert any(h % 2 for ins, _ in table.values() for h, _ in ins) and any(w % 2 for ins, _ in table.values() for _, w in ins)
    assert p16["44x36"][0] == [(44, 36), (22, 18), (11, 9)] and p16["8x8"][1] == (1, 1) and p16["9x11"][0][0] == (9, 11)
    assert p19["2x44x36"][1] == (2, 2) and p19["1x16x16"][1] == (1, 1)
    assert {c["B"] for c in L.VGG19_CASES.values()} == {1, 2}


def resized(net, name, run):
    imgs = L.case_images(net, name, run)
    case = L.VGG16_CASES[name] if net == "vgg16" else L.VGG19_CASES[name]
    if net == "vgg16" and imgs[0].shape[1] != 3:
        imgs = tuple(t.repeat(1, 3, 1, 1) for t in imgs)
    if case.get("resize"):
        imgs = tuple(torch.nn.functional.interpolate(t, size=(224, 224), mode="bilinear", align_corners=False) for t in imgs)
    return imgs


@pytest.mark.parametrize("run", [0, 1])
@pytest.mark.parametrize("name", list(L.VGG16_CASES))
def test_vgg16_cases_are_alive_and_two_branches_differ(name, run):
    w = vgg_ref.synth_vgg_weights()
    a, b = resized("vgg16", name, run)
    B = a.shape[0]
    acts = chain(L.normalise(torch.cat([a, b], 0), torch.float64), w, L.VGG16_ROWS, torch.float64)
    for i, y in enumerate(acts):
        assert y.max().item() > 0 and (y != 0).double().mean().item() >= 0.10, (name, i)
    for i in L.VGG16_SLICE_END:
        assert (acts[i][:B] - acts[i][B:]).abs().mean().item() > 0, (name, i)


@pytest.mark.parametrize("run", [0, 1])
@pytest.mark.parametrize("name", list(L.VGG19_CASES))
def test_vgg19_cases_are_alive_and_two_branches_differ(name, run):
    w = vgg_ref.synth_vgg19_weights()
    imgs = resized("vgg19", name, run)
    B = imgs[0].shape[0]
    acts = chain(L.normalise(torch.cat(imgs, 0), torch.float64), w, L.VGG19_ROWS, torch.float64)
    for i, y in enumerate(acts):
        assert y.max().item() > 0 and (y != 0).double().mean().item() >= 0.10, (name, i)
    c = acts[vgg_ref.VGG19_CONTENT_TAP]
    assert ((c[:B] - c[B:2 * B]) ** 2).mean().item() > 0
    for i in vgg_ref.VGG19_STYLE_TAPS:
        g = L.gram(acts[i], torch.float64)
        assert ((g[:B] - g[2 * B:]) ** 2).mean().item() > 0, (name, i)
