"""CPU: the detector's compute_dtype argument (fp32 / bf16 / f16) and the 16-bit restatement tests/detector16_ref.py, which with
the identity hook is tests/detector_ref.eager_forward."""
import os

import numpy as np
import pytest
import torch

from stlpose_amd import efficientdet as E
from tests import detector16_ref as R16
from tests import detector_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "detector", "g15_effdet.npz")


def _layout(cc):
    rows = bytes(np.load(FIX)[f"d{cc}_layout"]).decode().split("\n")
    return {k: tuple(int(v) for v in s.split(",") if v) for k, s in (r.split(" ") for r in rows)}


def test_compute_dtype_argument():
    models = {d: E.setup_detector("efficientdet", "d0", compute_dtype=d) for d in ("fp32", "bf16", "f16")}
    for d, m in models.items():
        assert m.compute_dtype == d
    assert E.setup_detector("efficientdet", "d0").compute_dtype == "fp32"
    assert E.EfficientDetBackbone(num_classes=1, compound_coef=0).compute_dtype == "fp32"
    with pytest.raises(ValueError, match="fp32.*bf16.*f16"):
        E.setup_detector("efficientdet", "d0", compute_dtype="int8")
    ref = [(k, v.dtype, tuple(v.shape)) for k, v in models["fp32"].state_dict().items()]
    assert [k for k, _, _ in ref] == list(_layout(0))
    for d in ("bf16", "f16"):
        assert [(k, v.dtype, tuple(v.shape)) for k, v in models[d].state_dict().items()] == ref
        assert all(p.dtype == torch.float32 for p in models[d].parameters())
        sd = R.synth_state_dict(_layout(0))
        models[d].load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)


def test_identity_hook_is_the_eager_forward():
    sd = R.synth_state_dict(_layout(0))
    x = R16.canvas()
    with torch.no_grad():
        want = R.eager_forward(sd, 0, 1, x)
        got = R16.forward16(sd, 0, 1, x)
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
