"""GPU: the VGG trunk (stlpose_amd/vgg.py::Trunk) link by link against the fp64 yardstick tests/vgg_layers_ref.py, read from the
plans of VGGPerceptualLoss (VGG16) and VGG19StyleLoss: every stored activation from the GPU's OWN stored input to that link, the
Gram matrices from the stored features, and the loss reductions from the stored activations / Gram matrices.  The end-to-end loss
scalars (test_vgg_gpu.py, test_vgg19_style_gpu.py) are means of differences between two branches through the same kernels: a fault
common to both cancels there, a localised one is averaged away (tests/test_vgg_layers_cpu.py shows the bounds here reject those).

Bounds (tests/vgg_layers_ref.py).  fp32 tensors: e = max|device - Y| / max|Y| <= max(MARGIN * e32, 1e-6), e32 the same figure of
torch's fp32 evaluation from the same input.  bf16 activations: for every element |device - Y| <= 2**-8 |Y| + max(MARGIN * e32,
1e-6) max|Y|, Y formed with the weights rounded to bf16 as stl_weight_prep rounds them.  MARGIN is 8, as in
tests/test_detector_train_gpu.py and for its reason (sums of thousands of terms in another order than torch's: MFMA tiles,
split-K slabs), except for the fp32 3x3 conv layers, which are held with MARGIN_CONV32 = 16: a correct kernel needs more than 8
at K = 9 * 512.  The conv carries one fp32 accumulator through all K products, whose rounding error grows as sqrt(K), while
torch's blocked sum stays at e32 = 2 .. 12 units of 2**-24 whatever K is; the reasoning is in tests/vgg_layers_ref.py.  With 8,
two of the 144 fp32 layer figures fail: 2x44x36, acts[10] (e 2.23e-6, e32 2.48e-7, ratio 9.01) and acts[11] of the second forward
(e 2.07e-6, e32 2.47e-7, ratio 8.36), both 512 -> 512 on the 5 x 4 maps.

The first link.  fp32: acts[0] is held from the fp64-normalised image (stl_patch3x3 with mean / std and the K = 32 1x1 conv in one
figure), and so is the patch tensor.  bf16: the plan stores the normalised patches in bf16, and the elementwise bound allows one
rounding of the OUTPUT only, so an exact conv on once-rounded patches does not meet it from the un-rounded image
(test_vgg_layers_cpu.py::test_first_link_in_bf16_is_two_links).  The link is therefore checked as the two it is: the stored
patches against the fp64-normalised image (elementwise bound; columns 27 .. 31 exactly 0), acts[0] from the stored patches.

Measured on the MI355X, e / e32 and the largest e per group:
* patches, fp32: bit-equal to torch's fp32 normalisation (ratio 1.00, e <= 9.7e-8); bf16: largest |error| / allowed 0.995,
  e <= 3.0e-3 (the rounding itself).
* acts[0] (K = 27), fp32, from the image and from the stored patches: 0.71 - 1.36, e <= 3.1e-7.
* layer activations fp32: 0.76 - 9.01, e <= 2.4e-6; by K = 576 / 1152 / 2304 / 4608 the ratio reaches 4.3 / 5.5 / 7.9 / 9.0 and
  e 1.2e-6 / 1.3e-6 / 2.1e-6 / 2.4e-6.
* layer activations bf16 (acts[0] included): largest |error| / allowed 0.995 over every element, e <= 3.8e-3: the bound is
  reached to within half a percent, as the rounding of a value just above a power of two does.
* Gram matrices: fp32 0.28 - 1.58 (e <= 3.0e-7), bf16 0.11 - 1.91 (e <= 1.1e-7; e32 = 0 for twelve Grams); every figure is below
  the 1e-6 floor; each Gram is symmetric to the same bound.
* reductions (VGG16 loss, VGG19 content and style): 0.07 - 1.24, e <= 8.2e-8, below the floor.
Each test takes under a second (the 224 x 224 case 0.9 s, nearly all of it the fp64 yardstick on the CPU).
"""
import pytest
import torch

from oracle import vgg_ref
from stlpose_amd import VGG19StyleLoss, VGGPerceptualLoss
from stlpose_amd.vgg import SLICE_END
from stlpose_amd.vgg19_style import CONTENT_TAP, STYLE_TAPS
from tests import vgg_layers_ref as L

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def nchw(buf, tdt, nb, dims):
    """A plan's uint8 activation buffer -> the stored NHWC tensor as NCHW on the CPU, in its own type."""
    h, w, c = dims
    return buf.view(tdt).reshape(nb, h, w, c).cpu().permute(0, 3, 1, 2).contiguous()


def snapshot(trunk):
    torch.cuda.synchronize()
    nb = trunk.img.shape[0]
    H, W = trunk.img.shape[2:]
    return dict(img=trunk.img.cpu().clone(), patches=trunk.keep[0].view(trunk.tdt).reshape(nb, H, W, 32).cpu().clone(),
                acts=[nchw(a, trunk.tdt, nb, d) for a, d in zip(trunk.acts, trunk.dims)])


@pytest.fixture(scope="module", params=[(n, dt) for n in L.VGG16_CASES for dt in ("fp32", "bf16")], ids=lambda p: f"{p[0]}-{p[1]}")
def vgg16_runs(request):
    """Two forwards of one module through ONE plan (different images) -> per run the stored tensors and the returned loss."""
    name, dt = request.param
    case = L.VGG16_CASES[name]
    w = vgg_ref.synth_vgg_weights()
    m = VGGPerceptualLoss(resize=case["resize"], state_dict=w, compute_dtype=dt).cuda()
    runs = []
    for run in (0, 1):
        a, b = L.case_images("vgg16", name, run)
        loss = m(a.cuda(), b.cuda())
        assert len(m._plans) == 1
        trunk, _ = next(iter(m._plans.values()))
        runs.append(dict(snapshot(trunk), loss=loss.cpu(), B=case["B"]))
    return dict(w=w, rows=L.VGG16_ROWS, dt=dt, runs=runs, name=name)


@pytest.fixture(scope="module", params=[(n, dt) for n in L.VGG19_CASES for dt in ("fp32", "bf16")], ids=lambda p: f"{p[0]}-{p[1]}")
def vgg19_runs(request):
    name, dt = request.param
    case = L.VGG19_CASES[name]
    w = vgg_ref.synth_vgg19_weights()
    m = VGG19StyleLoss(state_dict=w, compute_dtype=dt).cuda()
    runs = []
    for run in (0, 1):
        x, c, s = L.case_images("vgg19", name, run)
        total, closs, sloss = m(x.cuda(), c.cuda(), s.cuda())
        assert len(m._plans) == 1
        plan = next(iter(m._plans.values()))
        runs.append(dict(snapshot(plan.trunk), grams=[g.cpu() for g in plan.grams()], content=plan.content.cpu().clone(),
                         closs=closs.cpu(), sloss=sloss.cpu(), nsplit=[sl.shape[1] for sl, _ in plan.slabs], B=case["B"]))
    return dict(w=w, rows=L.VGG19_ROWS, dt=dt, runs=runs, name=name)


def check_links(ctx, run):
    """Every stored activation of one forward from the stored input of its link."""
    w, rows, bf16 = ctx["w"], ctx["rows"], ctx["dt"] == "bf16"
    r = ctx["runs"][run]
    tag = f"{ctx['name']} {ctx['dt']} run {run}"
    for i, y in enumerate(r["acts"]):
        assert torch.isfinite(y.float()).all(), (tag, i)
    wt = lambda i: (w[f"features.{rows[i][0]}.weight"], w[f"features.{rows[i][0]}.bias"])   # noqa: E731
    # -- the patch layer + conv1_1
    x64, x32 = L.normalise(r["img"], F64), L.normalise(r["img"], F32)
    stored = r["patches"][..., :27]
    assert (r["patches"][..., 27:] == 0).all(), tag
    if bf16:
        L.hold16(f"{tag} patches", stored, L.unfold3x3(x64), L.unfold3x3(x32))
        L.hold16(f"{tag} acts[0] from the stored patches", r["acts"][0], L.patch_layer(stored, *wt(0), F64, True),
                 L.patch_layer(stored.float(), *wt(0), F32, True))
    else:
        L.hold(f"{tag} patches", stored, L.unfold3x3(x64), L.unfold3x3(x32))
        L.hold(f"{tag} acts[0] from the image", r["acts"][0], L.layer(x64, *wt(0), False, F64), L.layer(x32, *wt(0), False, F32))
        L.hold(f"{tag} acts[0] from the stored patches", r["acts"][0], L.patch_layer(stored, *wt(0), F64), L.patch_layer(stored, *wt(0), F32))
    # -- layers 1 .. n-1 from the stored acts[i - 1]
    for i in range(1, len(rows)):
        xin, pool = r["acts"][i - 1], rows[i][1]
        y64, y32 = L.layer(xin, *wt(i), pool, F64, bf16), L.layer(xin, *wt(i), pool, F32, bf16)
        assert y64.shape == r["acts"][i].shape
        if bf16:
            L.hold16(f"{tag} acts[{i}]", r["acts"][i], y64, y32)
        else:
            L.hold(f"{tag} acts[{i}]", r["acts"][i], y64, y32, L.MARGIN_CONV32)


@pytest.mark.parametrize("run", [0, 1])
def test_vgg16_every_layer_from_its_stored_input(vgg16_runs, run):
    check_links(vgg16_runs, run)


@pytest.mark.parametrize("run", [0, 1])
def test_vgg19_every_layer_from_its_stored_input(vgg19_runs, run):
    check_links(vgg19_runs, run)


def test_vgg16_second_forward_rewrites_every_activation(vgg16_runs):
    a, b = vgg16_runs["runs"]
    assert not torch.equal(a["img"], b["img"]) and not torch.equal(a["patches"], b["patches"])
    for i, (p, q) in enumerate(zip(a["acts"], b["acts"])):
        assert not torch.equal(p, q), i


def test_vgg19_second_forward_rewrites_every_activation(vgg19_runs):
    a, b = vgg19_runs["runs"]
    for i, (p, q) in enumerate(zip(a["acts"], b["acts"])):
        assert not torch.equal(p, q), i
    for p, q in zip(a["grams"], b["grams"]):
        assert not torch.equal(p, q)


@pytest.mark.parametrize("run", [0, 1])
def test_vgg16_loss_from_stored_slice_ends(vgg16_runs, run):
    """stl_l1_partial + stl_sum_partials (accumulate 0, then 1 three times): the returned loss against sum_s mean |a - b|."""
    r = vgg16_runs["runs"][run]
    B = r["B"]
    ends = [r["acts"][i] for i in sorted(SLICE_END)]
    y64 = sum((f[:B].double() - f[B:].double()).abs().mean() for f in ends)
    y32 = sum((f[:B].float() - f[B:].float()).abs().mean() for f in ends)
    assert y64.item() > 0
    L.hold(f"{vgg16_runs['name']} {vgg16_runs['dt']} run {run} loss", r["loss"], y64, y32)


@pytest.mark.parametrize("run", [0, 1])
def test_vgg19_grams_from_stored_features(vgg19_runs, run):
    """Per tap and Gram image: the split-K slabs' sum against F F^T / (C H W) of the stored features.  The slabs are fp32 and
    the stored features exact inputs, so bf16 gets no rounding term."""
    r = vgg19_runs["runs"][run]
    B = r["B"]
    tag = f"{vgg19_runs['name']} {vgg19_runs['dt']} run {run}"
    imgs = list(range(B)) + list(range(2 * B, 3 * B))   # stylised and style images, in slab order
    for t, i in enumerate(STYLE_TAPS):
        f = r["acts"][i][imgs]
        g64, g32 = L.gram(f, F64), L.gram(f.float(), F32)
        got = r["grams"][t]
        assert got.shape == g64.shape and torch.isfinite(got).all()
        for j in range(len(imgs)):
            L.hold(f"{tag} gram tap {i} image {j}", got[j], g64[j], g32[j])
            sym = L.rel_err(got[j].t(), got[j])
            assert sym <= L.bound(L.rel_err(g32[j], g64[j])), (tag, i, j, sym)
    if vgg19_runs["name"] == "2x44x36":
        assert max(r["nsplit"]) > 1, r["nsplit"]   # the slab sum is exercised


@pytest.mark.parametrize("run", [0, 1])
def test_vgg19_losses_from_stored_features_and_grams(vgg19_runs, run):
    r = vgg19_runs["runs"][run]
    B = r["B"]
    tag = f"{vgg19_runs['name']} {vgg19_runs['dt']} run {run}"
    f = r["acts"][CONTENT_TAP]
    c64 = ((f[:B].double() - f[B:2 * B].double()) ** 2).mean()
    c32 = ((f[:B].float() - f[B:2 * B].float()) ** 2).mean()
    assert c64.item() > 0 and torch.equal(r["content"], r["closs"])
    L.hold(f"{tag} content (stl_l2_partial)", r["closs"], c64, c32)
    s64 = sum(((g[:B] - g[B:]) ** 2).mean() for g in r["grams"])
    s32 = sum(((g[:B].float() - g[B:].float()) ** 2).mean() for g in r["grams"])
    assert s64.item() > 0
    L.hold(f"{tag} style", r["sloss"], s64, s32)
