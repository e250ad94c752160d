"""CPU: the restated detection loss (tests/detector_train_ref.py) on a case worked out by hand, the folded-to-raw chain rule of
stlpose_amd/detector_train.py against autograd of the eager layer, and the validation of ``targets``."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stlpose_amd import detector_train as T
from stlpose_amd.efficientdet import resize_meta
from tests import detector_train_ref as TR


def test_restated_loss_on_a_hand_computed_case():
    """One box (0, 0) - (10, 10) and four anchors: the box itself (IoU 1, positive), its left 45 % (IoU 0.45, ignored), its left
    30 % (IoU 0.3, negative), a far one (IoU 0, negative); a second image without boxes (every anchor negative)."""
    anchors = torch.tensor([[0, 0, 10, 10], [0, 0, 10, 4.5], [0, 0, 10, 3], [20, 20, 30, 30]], dtype=torch.float64)   # y1, x1, y2, x2
    gt = torch.tensor([[0, 0, 10, 10, 0]], dtype=torch.float64)
    offsets = [0, 1, 1]
    cls = torch.tensor([[[0.8], [0.3], [0.2], [0.00001]], [[0.1], [0.5], [0.99999], [0.4]]], dtype=torch.float64)
    reg = torch.zeros(2, 4, 4, dtype=torch.float64)
    reg[0, 0] = torch.tensor([0.05, 0.0, 0.5, -0.1], dtype=torch.float64)   # the target is (0, 0, 0, 0): the box is the anchor
    c, r, npos, state = TR.detection_loss(reg, cls, anchors, gt, offsets)
    assert npos == [1, 0]
    assert state.tolist() == [[1, -1, 0, 0], [0, 0, 0, 0]]
    neg = lambda p: 0.75 * p ** 2 * -math.log(1 - p)  # noqa: E731
    lo, hi = 1e-4, 1 - 1e-4
    c0 = (0.25 * 0.2 ** 2 * -math.log(0.8) + neg(0.2) + neg(lo)) / 1     # the ignored anchor adds nothing; 1e-5 is clamped to 1e-4
    c1 = (neg(0.1) + neg(0.5) + neg(hi) + neg(0.4)) / 1                   # no positives: divided by max(0, 1)
    assert c.item() == pytest.approx((c0 + c1) / 2, rel=1e-12)
    l0 = (4.5 * 0.05 ** 2 + 0.0 + (0.5 - 1 / 18) + 4.5 * 0.1 ** 2) / 4     # 0.5 > 1/9: the linear branch
    assert r.item() == pytest.approx(50.0 * (l0 + 0.0) / 2, rel=1e-12)
    # the gradient with respect to the pre-sigmoid output is zero where the clamp is active and on the ignored anchor
    _, _, dreg, dlogit, _, _ = TR.loss_and_output_grads(reg, cls, anchors, gt, offsets, torch.float64)
    assert dlogit[0, 1, 0] == 0 and dlogit[0, 3, 0] == 0 and dlogit[1, 2, 0] == 0 and dlogit[0, 0, 0] < 0 < dlogit[0, 2, 0]
    assert (dreg[0, 0] != 0).tolist() == [True, False, True, True] and not dreg[0, 1:].any() and not dreg[1].any()
    assert dreg[0, 0, 2].item() == pytest.approx(50.0 / (2 * 4), rel=1e-12)


def test_first_argmax_and_degenerate_boxes():
    anchors = torch.tensor([[0, 0, 10, 10]], dtype=torch.float64)
    gt = torch.tensor([[0, 0, 10, 8, 0], [0, 2, 10, 10, 1], [5, 5, 5, 5, 0]], dtype=torch.float64)   # two ties at 0.8, one empty box
    state, g, m = TR.assign(anchors, gt)
    assert state.tolist() == [1] and g.tolist() == [0] and m.item() == pytest.approx(0.8)


@pytest.mark.parametrize("ci,co", [(64, 64), (160, 160), (24, 36)])
def test_fold_chain_matches_autograd_of_the_eager_layer(ci, co):
    """W' = W s, b' = b s + t: the gradients of the folded tensors, carried to W, b, gamma, beta by fold_chain, equal autograd's
    through F.conv2d + eval-mode F.batch_norm."""
    g = torch.Generator().manual_seed(ci + co)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    W, b, gamma, beta, mean = rnd(co, ci).requires_grad_(), rnd(co).requires_grad_(), rnd(co).requires_grad_(), rnd(co).requires_grad_(), rnd(co)
    var = torch.rand(co, generator=g, dtype=torch.float64) + 0.5
    x, dy = rnd(3, ci, 5, 4), rnd(3, co, 5, 4)
    y = F.batch_norm(F.conv2d(x, W[:, :, None, None], b), mean, var, gamma, beta, False, 0.0, 1e-3)
    (y * dy).sum().backward()
    xm, dm = x.permute(0, 2, 3, 1).reshape(-1, ci), dy.permute(0, 2, 3, 1).reshape(-1, co)
    GW, Gb = dm.t() @ xm, dm.sum(0)   # what the weight-gradient kernel returns for the folded layer
    dW, db, dgamma, dbeta = T.fold_chain(W.detach(), b.detach(), gamma.detach(), mean, var, 1e-3, GW, Gb)
    for got, want in ((dW, W.grad), (db, b.grad), (dgamma, gamma.grad), (dbeta, beta.grad)):
        assert TR.rel_err(got, want) < 1e-12


def test_targets_are_validated_and_scaled_to_the_canvas():
    sizes = [(300, 400), (480, 360)]
    ok = [{"boxes": torch.tensor([[40.0, 30.0, 200.0, 150.0], [0.0, 0.0, 400.0, 300.0]]), "labels": torch.tensor([1, 2])},
          {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}]
    gt, off = T.pack_targets(ok, sizes, 2)
    assert off.tolist() == [0, 2, 2] and gt.dtype == np.float32 and gt.shape == (2, 5)
    new_w, new_h = resize_meta(300, 400)[:2]
    sx, sy = new_w / 400, new_h / 300
    np.testing.assert_allclose(gt[0], [40 * sx, 30 * sy, 200 * sx, 150 * sy, 0], rtol=1e-7)
    assert gt[1, 4] == 1 and gt[1, 2] == np.float32(512)

    def bad(i, **kw):
        t = [dict(d) for d in ok]
        t[i].update(kw)
        return t
    for targets, n in ((bad(0, boxes=torch.zeros(2, 5)), 2), (bad(0, boxes=torch.zeros(3, 4)), 2), (bad(0, boxes=torch.zeros(8)), 2),
                       (bad(0, labels=torch.tensor([[1, 1]])), 2), (bad(0, labels=torch.tensor([0, 1])), 2),
                       (bad(0, labels=torch.tensor([1, 3])), 2), (bad(0, labels=torch.tensor([1.0, 1.0])), 2),
                       (bad(1, labels=torch.tensor([1])), 2), (ok[:1], 2), ([ok[0], None], 2), ([ok[0], {"boxes": torch.zeros(0, 4)}], 2)):
        with pytest.raises(ValueError, match="detection_loss"):
            T.pack_targets(targets, sizes, n)
    with pytest.raises(ValueError, match=r"1 \.\. 1"):
        T.pack_targets(ok, sizes, 1)   # label 2 with one class


def test_detection_loss_is_fp32_only():
    from stlpose_amd.efficientdet import EfficientDetBackbone
    m = EfficientDetBackbone(num_classes=1, compound_coef=0, compute_dtype="bf16")
    with pytest.raises(NotImplementedError, match="fp32"):
        m.detection_loss(torch.zeros(1, 3, 64, 64), [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}])
