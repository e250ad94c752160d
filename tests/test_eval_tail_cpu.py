"""No GPU: the numpy yardstick of the fused evaluation tail (tests/eval_tail_ref.py) against the oracle's own pieces, the host
arithmetic of the PCK (pose_parsing.pck_from_coords) against oracle.pose_ref.pck_accuracy, and the public surface."""
import numpy as np
import pytest
import torch

from oracle import pose_ref
from tests import eval_tail_ref as R


@pytest.fixture(scope="module", params=R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def batch(request):
    a, bf, t, tw = R.case(request.param, seed=3)
    return a, bf, t, tw, R.tail(a, bf, t, tw)


def test_yardstick_equals_the_oracle_pieces(batch):
    a, bf, t, tw, y = batch
    b, j, h, w = a.shape
    # flip_back + shift + average (pose_ref.forward_pass behind its two forwards); the oracle swaps all eight pairs, so J = 17
    if j == 17:
        of = pose_ref.flip_back(bf)
        shifted = of.copy()
        shifted[:, :, :, 1:] = of[:, :, :, :-1]
        assert np.array_equal(y["merged"], (a + shifted) * np.float32(0.5))
    assert y["merged"].dtype == np.float32
    # arg-max with the mask rule
    for hm, xy in ((y["merged"], y["pred_xy"]), (t, y["tgt_xy"])):
        want, mx = pose_ref.get_max_preds(hm)
        assert np.array_equal(xy, want)
    assert np.array_equal(y["maxval"], pose_ref.get_max_preds(y["merged"])[1][..., 0])
    # refinement and inverse crop transform: the refined coordinates exactly; the image coordinates to float32 rounding (the
    # oracle multiplies by 1 / s in fp64 where the kernels divide by s: a few fp64 ulps, then one cast to float32)
    rng = np.random.Generator(np.random.PCG64(1))
    c, s = (rng.random((b, 2)) * 300 + 100).astype(np.float32), (rng.random((b, 2)) + 0.5).astype(np.float32)
    preds, mx, coords = pose_ref.final_preds(y["merged"], c, s)
    assert np.array_equal(y["coords"], coords)
    got = R.affine(y["coords"], y["maxval"], c, s, h, w)
    assert got.dtype == np.float32 and np.array_equal(got[..., 2], mx[..., 0])
    assert np.allclose(got[..., :2], preds, rtol=2.0 ** -22, atol=0)
    # loss: the oracle sums fp32 products in fp32, so only to fp32 summation error
    want = float(pose_ref.person_mse_loss(torch.from_numpy(y["merged"]), torch.from_numpy(t), torch.from_numpy(tw)))
    assert abs(y["loss"] - want) <= 1e-5 * want


def test_yardstick_without_a_mirrored_pass():
    a, _, t, tw = R.case((2, 17, 8, 6), seed=5)
    y = R.tail(a, None, t, tw)
    assert np.array_equal(y["merged"], a) and np.array_equal(y["pred_xy"], pose_ref.get_max_preds(a)[0])


def test_nan_is_the_argmax():
    a, bf, t, tw = R.case((1, 17, 8, 6), seed=7, nan=True)
    y = R.tail(a, bf, t, tw)
    assert np.isnan(y["maxval"][0, 16]) and np.array_equal(y["pred_xy"][0, 16], [0, 0]) and np.isnan(y["loss"])


def _pck_case(seed):
    a, bf, t, tw = R.case((4, 17, 12, 10), seed=seed)
    y = R.tail(a, bf, t, tw)
    return y, t


def test_pck_from_coords_equals_the_oracle():
    from stlpose_amd.pose_parsing import pck_from_coords
    for seed in (0, 1):
        y, t = _pck_case(seed)
        acc, avg, cnt, _ = pose_ref.pck_accuracy(y["merged"], t)
        got = pck_from_coords(y["pred_xy"], y["tgt_xy"], 12, 10)
        assert np.array_equal(got[0], acc) and got[1] == avg and got[2] == cnt
    # a joint without a valid target in the whole batch: -1, and out of the average
    out, tgt = np.zeros((2, 3, 12, 10), np.float32), np.zeros((2, 3, 12, 10), np.float32)
    out[:, :, 5, 5] = 1
    tgt[:, 0, 5, 5] = tgt[:, 2, 6, 5] = 1
    tgt[:, 1, 1, 7] = 1   # y = 1 is not above 1
    got = pck_from_coords(R.max_preds(out)[0], R.max_preds(tgt)[0], 12, 10)
    want = pose_ref.pck_accuracy(out, tgt)
    assert want[0][2] == -1 and want[2] == 2
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    # a distance of exactly 0.5 is not below the threshold: H = W = 40, so both axes are normalised by 4, and dx = 2
    out, tgt = np.zeros((1, 2, 40, 40), np.float32), np.zeros((1, 2, 40, 40), np.float32)
    out[0, 0, 10, 12] = tgt[0, 0, 10, 10] = 1      # dx = 2: 0.5, a miss
    out[0, 1, 10, 11] = tgt[0, 1, 10, 10] = 1      # dx = 1: 0.25, a hit
    got = pck_from_coords(R.max_preds(out)[0], R.max_preds(tgt)[0], 40, 40)
    want = pose_ref.pck_accuracy(out, tgt)
    assert list(want[0]) == [0.5, 0.0, 1.0]
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] == 0.5


def test_public_surface():
    from stlpose_amd import ops
    from stlpose_amd.evaluate import Evaluator
    with pytest.raises(ValueError, match="tail 'x'"):
        Evaluator(None, tail="x")
    assert Evaluator(None).tail == "host"
    assert "eval_tail" in ops.OPS and "eval_affine" in ops.OPS


def test_ops_are_gpu_only_and_traceable():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.stlpose.eval_affine(torch.zeros(1, 17, 2), torch.zeros(1, 17), torch.zeros(1, 2), torch.zeros(1, 2), 8, 6)
    with FakeTensorMode():
        hm = torch.empty(2, 17, 8, 6, device="cuda")
        tabs = [torch.empty(4, 17, 2, device="cuda") for _ in range(3)] + [torch.empty(4, 17, device="cuda")]
        assert torch.ops.stlpose.eval_tail(hm, None, torch.empty(17, dtype=torch.int32, device="cuda"), hm, torch.empty(2, 17, 1, device="cuda"),
                                           *tabs, torch.empty(34, dtype=torch.float64, device="cuda"), torch.empty(4, device="cuda"), 0, 0) is None
        preds = torch.ops.stlpose.eval_affine(tabs[2], tabs[3], torch.empty(3, 2, device="cuda"), torch.empty(3, 2, device="cuda"), 8, 6)
        assert preds.shape == (3, 17, 3)
