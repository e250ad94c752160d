"""CPU: the split-bf16 conv mode ("fp32x3": fp32 tensors multiplied as two bf16 pieces each, three products) without a device.

What the split itself guarantees, that the yardstick (tests/split_ref.py) passes the parity bars the device mode is held to in
tests/test_fp32x3_gpu.py -- so those bars are reachable --, that the per-launch bound tells the three-product kernel from plain
fp32 and from a two-product kernel, and the host side of the mode: the ABI field, the dtype names, the plans."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hrnet_ref, pose_ref, vgg_ref
from tests.golden.make_golden import synth_batch
from tests.split_ref import LAUNCH_CASES, bf16x3, conv_x3, conv_x3_fp32, launch_case, split_bf16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------- the split
def _values():
    g = torch.Generator().manual_seed(7)
    rnd = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-30, 30, (1 << 16,), generator=g).float())
    few = torch.tensor([1.0, -1.0, 0.5, 3.0, 1.5, 257.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -15), 65280.0, 2.0 ** -100])
    return {"random": rnd, "few_bits": few, "zeros": torch.tensor([0.0, -0.0])}


@pytest.mark.parametrize("kind", ["random", "few_bits", "zeros"])
def test_split_properties(kind):
    x = _values()[kind]
    hi, lo = split_bf16(x)
    assert torch.equal(hi, x.to(torch.bfloat16).float())
    assert torch.equal(lo.to(torch.bfloat16).float(), lo), "lo is not a bf16 number"
    err = ((hi.double() + lo.double()) - x.double()).abs()
    assert bool((err <= 2.0 ** -16 * x.double().abs()).all()), float((err / x.double().abs().clamp_min(1e-300)).max())
    print(f"split {kind}: max |hi + lo - x| / |x| = {float((err / x.double().abs().clamp_min(1e-300)).max()):.3e} (bar 2^-16 = {2.0 ** -16:.3e})")
    if kind == "zeros":
        assert torch.equal(hi, torch.zeros(2)) and torch.equal(lo, torch.zeros(2))
    if kind == "few_bits":   # numbers of at most 8 significant bits are their own hi
        exact = x.to(torch.bfloat16).float() == x
        assert bool((lo[exact] == 0).all())
    # the third piece brings the split to fp32's own precision
    h3, m3, l3 = split_bf16(x, 3)
    assert torch.equal(h3, hi) and torch.equal(m3, lo)
    assert bool((((h3.double() + m3.double() + l3.double()) - x.double()).abs() <= 2.0 ** -24 * x.double().abs()).all())


# ---------------------------------------------------------------------------------------- the yardstick passes the device's bars
def _synth(arch):
    return hrnet_ref.load_synth(hrnet_ref.RefPoseNet(arch)).eval()


def test_yardstick_tiny_eval_meets_g1():
    g = np.load(os.path.join(GOLDEN, "g1_tiny_eval.npz"))
    m = _synth("tiny")
    with torch.no_grad(), bf16x3(m):
        out = m(torch.from_numpy(g["img"])).numpy()
    err = np.abs(out - g["output"]).max() / np.abs(g["output"]).max()
    print(f"tiny eval under bf16x3 vs G1: {err:.3e} of max (bar 1e-3)")
    assert 0 < err < 1e-3   # 0: the context manager swapped nothing
    with torch.no_grad():   # ... and put everything back
        assert np.array_equal(m(torch.from_numpy(g["img"])).numpy(), _synth("tiny")(torch.from_numpy(g["img"])).detach().numpy())
    assert all("forward" not in mod.__dict__ for mod in m.modules())


def test_yardstick_w32_flip_test_meets_g3():
    g = np.load(os.path.join(GOLDEN, "g3_w32_256x192.npz"))
    img, _, _ = synth_batch(2, 256, 192, seed=1234, sigma=2.0)
    m = _synth("w32")
    with torch.no_grad(), bf16x3(m):
        of = pose_ref.forward_pass(m, torch.from_numpy(img), flip=True).numpy()
    err = np.abs(of.reshape(-1)[::64] - g["flip_sample"]).max() / np.abs(g["flip_sample"]).max()
    pf, _ = pose_ref.get_max_preds(of)
    print(f"W32 256x192 flip test under bf16x3 vs G3: {err:.3e} of max (bar 1e-3), argmax differing {int((pf != g['flip_argmax_xy']).any(-1).sum())} of {pf.shape[0] * pf.shape[1]}")
    assert err < 1e-3
    assert np.array_equal(pf, g["flip_argmax_xy"])


def test_yardstick_w48_eval_meets_g8():
    g = np.load(os.path.join(GOLDEN, "g8_w48.npz"))
    img, _, _ = synth_batch(1, 128, 96, seed=5)
    m = _synth("w48")
    with torch.no_grad(), bf16x3(m):
        out = m(torch.from_numpy(img)).numpy()
    ref = g["out_sample"]
    err = np.abs(out.reshape(-1)[::16] - ref).max() / np.abs(ref).max()
    print(f"W48 eval under bf16x3 vs G8: {err:.3e} of max (bar 1e-3)")
    assert err < 1e-3


@pytest.mark.parametrize("tag", ["rs_rgb", "rs_gray", "nr_rgb", "nr_odd", "nr_gray"])
def test_yardstick_vgg_loss_meets_g10(tag):
    g = np.load(os.path.join(GOLDEN, "g10_vgg.npz"))
    w = vgg_ref.synth_vgg_weights()
    a, b = torch.from_numpy(g[f"{tag}_in"]), torch.from_numpy(g[f"{tag}_tg"])
    with torch.no_grad(), bf16x3(vgg_ref):
        assert vgg_ref.F.conv2d is not F.conv2d and vgg_ref.F.relu is F.relu
        got = vgg_ref.vgg_perceptual_loss(a, b, w, resize=bool(g[f"{tag}_resize"])).item()
    assert vgg_ref.F is F, "bf16x3 left oracle.vgg_ref patched"
    ref = float(g[f"{tag}_loss"])
    print(f"VGG16 perceptual loss {tag} under bf16x3 vs G10: {abs(got - ref) / abs(ref):.3e} relative (bar 1e-3)")
    assert abs(got - ref) <= 1e-3 * abs(ref)


# ---------------------------------------------------------------------------------------- the per-launch bound separates
@pytest.mark.parametrize("name", [c[0] for c in LAUNCH_CASES])
def test_launch_bound_separates_three_products_from_fp32_and_from_two_products(name):
    x, w, stride, padding, y, bound = launch_case(name)
    scale = float(y.abs().max())
    rel = lambda t: float((t.double() - y).abs().max()) / scale   # noqa: E731
    three, plain, two = rel(conv_x3_fp32(x, w, stride, padding)), rel(F.conv2d(x, w, None, stride, padding)), rel(conv_x3(x, w, stride, padding, drop_lo_hi=True))
    print(f"{name}: bound {bound:.3e}; three products in fp32 {three / bound:.3f} x, plain fp32 {plain / bound:.2f} x, without lo*hi {two / bound:.0f} x")
    assert three <= bound
    assert plain > bound
    assert two > 100 * bound


# ---------------------------------------------------------------------------------------- host side of the mode
def test_abi_math_field_and_constants():
    from stlpose_amd import capi
    assert capi.MATH_NATIVE == 0 and capi.MATH_BF16X3 == 1
    assert capi.MATH.constants == {"STL_MATH_NATIVE": 0, "STL_MATH_BF16X3": 1}   # include/stlpose_hip_math.h
    names = [f[0] for f in capi.Conv._fields_]
    assert "math" in names and "pad_" not in names
    assert names.index("math") == names.index("ydtype") + 1 == len(names) - 1
    assert capi.Conv.math.offset == capi.Conv.ydtype.offset + 4 and capi.Conv.math.size == 4
    assert C.sizeof(capi.Conv) == capi.Conv.math.offset + 4, "the field fills the former padding: the layout did not change"
    assert capi.Conv().math == capi.MATH_NATIVE   # every zero-filled descriptor


def test_dtype_names(monkeypatch):
    from stlpose_amd import PoseHighResolutionNet, VGGPerceptualLoss, capi
    from stlpose_amd.adain import AdaINStylizer
    from stlpose_amd.efficientdet import EfficientDetBackbone
    from stlpose_amd.stylise import GatysStylizer
    from stlpose_amd.vgg19_style import VGG19StyleLoss
    m = PoseHighResolutionNet("w32", "fp32x3")
    assert m.compute_dtype == capi.F32X3 and capi.math_of(m.compute_dtype) == capi.MATH_BF16X3 and (m.compute_dtype & 0xffff) == capi.F32
    assert capi.math_of(PoseHighResolutionNet("tiny", "fp32").compute_dtype) == 0 and capi.math_of(capi.MIXED) == 0
    monkeypatch.setenv("STLPOSE_DTYPE", "fp32x3")
    assert PoseHighResolutionNet("tiny").compute_dtype == capi.F32X3
    with pytest.raises(ValueError):
        PoseHighResolutionNet("w32", "fp32x2")
    v = VGGPerceptualLoss(compute_dtype="fp32x3")
    assert v.dtype == capi.F32 and v.math == capi.MATH_BF16X3
    assert VGGPerceptualLoss(compute_dtype="fp32").math == 0 and VGGPerceptualLoss(compute_dtype="bf16").math == 0
    for build in (lambda: VGG19StyleLoss(compute_dtype="fp32x3"), lambda: GatysStylizer({}, compute_dtype="fp32x3"),
                  lambda: AdaINStylizer(compute_dtype="fp32x3"), lambda: EfficientDetBackbone(num_classes=1, compound_coef=0, compute_dtype="fp32x3")):
        with pytest.raises(ValueError):
            build()


def test_training_is_refused_at_construction():
    from stlpose_amd import PoseHighResolutionNet
    from stlpose_amd.engine import Engine
    from stlpose_amd.train_step import TrainStep
    from stlpose_amd.trainer import Trainer
    exp = {"training": {"num_epochs": 1, "save_frequency": 1}, "dataset": {"image_size": [64, 64]}}
    for build in (lambda: Trainer("/nonexistent", exp, [], [], 2, arch="tiny", compute_dtype="fp32x3"),
                  lambda: TrainStep(PoseHighResolutionNet("tiny", "fp32x3"), 2, 64, 64, device="cpu")):
        with pytest.raises(NotImplementedError, match='compute_dtype="fp32"') as e:
            build()
        assert "third bf16 piece" in str(e.value)
    m = PoseHighResolutionNet("tiny", "fp32x3")
    m._pack(torch.device("cpu"))
    for training, input_grad in ((True, False), (False, True)):
        with pytest.raises(NotImplementedError, match="third bf16 piece"):
            Engine(m.arch, m._store, 2, 64, 64, m.compute_dtype, training, input_grad)


def test_hrnet_plan_equals_fp32_plan_except_math():
    """The eval plan of the tiny net and of W32, built on the CPU (nothing is launched): launch for launch the fp32 plan, with
    ``math`` set on the conv launches and nowhere else.  Every other field is equal, the planned block shape and tile included;
    pointers (each plan has its own buffers) count as null or not."""
    from stlpose_amd import PoseHighResolutionNet, capi
    for arch, hw in (("tiny", (64, 64)), ("w32", (256, 192))):
        plans = {}
        for dt in ("fp32", "fp32x3"):
            m = PoseHighResolutionNet(arch, dt)
            m._pack(torch.device("cpu"))
            plans[dt] = m.engine(2, hw[0], hw[1], False).fwd_ops
        a, b = plans["fp32"], plans["fp32x3"]
        assert [o.name for o in a] == [o.name for o in b] and [o.stream for o in a] == [o.stream for o in b]
        nconv = 0
        for oa, ob in zip(a, b):
            assert type(oa.desc) is type(ob.desc)
            if not isinstance(oa.desc, capi.Conv):
                continue
            nconv += 1
            assert oa.desc.math == capi.MATH_NATIVE and ob.desc.math == capi.MATH_BF16X3
            for f, _ in capi.Conv._fields_:
                va, vb = getattr(oa.desc, f), getattr(ob.desc, f)
                if f in ("math", "src", "mask_bn"):
                    continue
                if getattr(capi.Conv, f).size == 8:   # a pointer: null in both or in neither
                    assert bool(va) == bool(vb), f
                else:
                    assert va == vb, (f, va, vb)
            assert (oa.desc.src.mode, oa.desc.src.relu, oa.desc.src.eps) == (ob.desc.src.mode, ob.desc.src.relu, ob.desc.src.eps)
        assert nconv > 20


def test_vgg_plan_equals_fp32_plan_except_math():
    from stlpose_amd import capi, vgg
    from tests import launch_plans
    ops = {}
    for dt in ("fp32", "fp32x3"):
        m = vgg.VGGPerceptualLoss(resize=False, compute_dtype=dt)
        vgg.ready(m, launch_plans.CPU)
        ops[dt] = m._plan(2, 32, 32, launch_plans.CPU)[0].ops
    a, b = list(ops["fp32"]), list(ops["fp32x3"])
    assert launch_plans.signature(a)["names"] == launch_plans.signature(b)["names"]
    nconv = 0
    for ea, eb in zip(a, b):
        name, args_a, args_b = ea[-2], ea[-1], eb[-1]
        if name != "stl_conv_forward":
            assert launch_plans.signature([ea]) == launch_plans.signature([eb])
            continue
        nconv += 1
        pa, pb = args_a[0]._obj, args_b[0]._obj
        assert (pa.math, pb.math) == (capi.MATH_NATIVE, capi.MATH_BF16X3)
        pb.math = 0
        assert launch_plans.signature([ea]) == launch_plans.signature([eb])
        pb.math = capi.MATH_BF16X3
    assert nconv == 10
