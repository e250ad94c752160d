"""CPU: the 16-bit fine-tuning yardstick (tests/detector_train16_ref.py) with identity stores against tests/detector_train_ref.py, the
bf16 transposed pack of the pointwise data gradient, and the compute_dtype gate of ``detection_loss``."""
import pytest
import torch

from stlpose_amd import efficientdet as E
from tests import detector_ref as R, detector_train16_ref as TR16, detector_train_ref as TR


def _small_case(dtype):
    """D0 heads on five tiny feature maps (4 x 4 down to 1 x 1); one box per level, the first anchor of that level's first cell."""
    m = E.EfficientDetBackbone(num_classes=1, compound_coef=0)
    sd = R.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    g = torch.Generator().manual_seed(3)
    sizes = (4, 2, 2, 1, 1)
    levels = [torch.randn(2, 64, h, h, generator=g).to(torch.float16).to(dtype) for h in sizes]
    rows, first = [], []
    for h, stride in zip(sizes, (8, 16, 32, 64, 128)):   # nine square anchors per cell, (y1, x1, y2, x2)
        first.append(len(rows))
        for y in range(h):
            for x in range(h):
                for a in range(9):
                    half = stride * (1.5 + 0.25 * a)
                    cy, cx = (y + 0.5) * stride, (x + 0.5) * stride
                    rows.append([cy - half, cx - half, cy + half, cx + half])
    anchors = torch.tensor(rows, dtype=torch.float32)
    gt = torch.cat([anchors[first], torch.zeros(5, 1)], 1)   # squares: (y1, x1, y2, x2) reads the same as (x1, y1, x2, y2)
    return sd, levels, anchors, gt, [0, 5, 5]


def test_identity_stores_reproduce_the_fp32_files_yardstick_bit_for_bit():
    for dtype in (torch.float64, torch.float32):
        sd, levels, anchors, gt, offsets = _small_case(dtype)
        want = TR.method_yardstick(sd, 0, 1, levels, anchors, gt, offsets, dtype)
        got = TR16.method_yardstick(sd, 0, 1, levels, anchors, gt, offsets, dtype)
        assert sum(want[5]) >= 4, want[5]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[5] == want[5]
        assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
        assert set(got[2]) == set(want[2])
        for k in want[2]:
            assert want[2][k].abs().max() > 0, k
            assert torch.equal(got[2][k], want[2][k]), k


def test_device_stores_change_every_gradient_but_little():
    """The hooks are live: with the device's roundings every gradient moves, by no more than a few bf16 units of its largest element."""
    sd, levels, anchors, gt, offsets = _small_case(torch.float64)
    want = TR.method_yardstick(sd, 0, 1, levels, anchors, gt, offsets, torch.float64)
    got = TR16.method_yardstick(sd, 0, 1, levels, anchors, gt, offsets, torch.float64, TR16.device_stores())
    assert got[5] == want[5]
    for k in want[2]:
        e = TR.rel_err(got[2][k], want[2][k])
        assert 0 < e < 0.05, (k, e)


@pytest.mark.parametrize("ci,co", [(64, 64), (160, 160), (64, 9), (160, 36)])
def test_transposed_pack_unpacks_to_the_bf16_rounded_transpose(ci, co):
    g = torch.Generator().manual_seed(ci + co)
    w = torch.randn(co, ci, generator=g, dtype=torch.float64) / ci ** 0.5
    wt, kp, np_ = E.pack_transposed(w)
    assert wt.dtype == torch.bfloat16 and kp == -(-co // 32) * 32 and np_ == -(-ci // 64) * 64 and wt.numel() == kp * np_
    assert torch.equal(E.unpack_transposed(wt, ci, co), w.t().to(torch.bfloat16))
    # the layout the header states: element ((kt * (Kp / 32) + ns) * 64 + 16 g + r) * 8 + i is W'[k = 16 kt + r][n = 32 ns + 8 g + i]
    full = torch.zeros(np_, kp, dtype=torch.float64)
    full[:ci, :co] = w.t()
    for kt, ns, gq, r, i in ((0, 0, 0, 0, 0), (np_ // 16 - 1, kp // 32 - 1, 3, 15, 7), (1, 0, 2, 5, 3)):
        e = ((kt * (kp // 32) + ns) * 64 + 16 * gq + r) * 8 + i
        assert wt[e] == full[16 * kt + r, 32 * ns + 8 * gq + i].to(torch.bfloat16)
    assert wt.double().abs().sum() == w.t().to(torch.bfloat16).double().abs().sum()   # the padding is zero (bf16 values add exactly in fp64)


def test_packer_adds_the_transposed_pieces_without_moving_the_forward_ones():
    m = E.EfficientDetBackbone(num_classes=1, compound_coef=0, compute_dtype="f16")
    plain, withT = E._Packer(torch.float16), E._Packer(torch.float16, transposed=True)
    a, b = m._pack_heads(plain), m._pack_heads(withT)
    assert a == b and plain.n == withT.n and plain.n16 == withT.n16 and not plain.partsT
    assert all(torch.equal(x, y) for x, y in zip(plain.parts16, withT.parts16))
    pws = [pk for h in ("regressor", "classifier") for pk in [a[h]["hpw"]] + [q for lv in a[h]["pw"] for q in lv]]
    assert sorted(withT.tmap) == sorted(pk[0] for pk in pws) and len(withT.partsT) == len(pws) == 2 * (1 + 5 * 3)
    conv = m.regressor.header.pointwise_conv.conv
    off, kt, nt = withT.tmap[a["regressor"]["hpw"][0]]
    wt = torch.cat(withT.partsT)[off:off + kt * nt]
    assert torch.equal(E.unpack_transposed(wt, 64, 36), conv.weight.detach().double().reshape(36, 64).t().to(torch.bfloat16))


def test_f16_passes_the_compute_dtype_gate():
    """f16 now trains: without a GPU the call fails where the fp32 model's does (no device), not at the gate; bf16 still stops there
    and names both modes that train."""
    args = (torch.zeros(1, 3, 64, 64), [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}])
    if torch.cuda.is_available():   # with a device the call goes through
        loss = E.EfficientDetBackbone(num_classes=1, compound_coef=0, compute_dtype="f16").detection_loss(*args)
        assert set(loss) == {"classification", "regression"}
        return
    errs = {}
    for mode in ("fp32", "f16"):
        with pytest.raises(Exception) as ei:
            E.EfficientDetBackbone(num_classes=1, compound_coef=0, compute_dtype=mode).detection_loss(*args)
        errs[mode] = ei.value
    assert not isinstance(errs["f16"], NotImplementedError), errs["f16"]
    assert type(errs["f16"]) is type(errs["fp32"]) and str(errs["f16"]) == str(errs["fp32"])
    with pytest.raises(NotImplementedError, match=r"fp32.*f16"):
        E.EfficientDetBackbone(num_classes=1, compound_coef=0, compute_dtype="bf16").detection_loss(*args)
