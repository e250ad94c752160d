"""GPU, BASELINE.json full sizes (W32, 384x288, batch 32, bf16): size-independent properties."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from stlpose_amd import PoseHighResolutionNet  # noqa: E402
from stlpose_amd.train_step import TrainStep  # noqa: E402


def _batch(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, H, W, generator=g)
    hh, ww = H // 4, W // 4
    cx = torch.randint(0, ww, (B, 17, 1, 1), generator=g).float()
    cy = torch.randint(0, hh, (B, 17, 1, 1), generator=g).float()
    ys, xs = torch.arange(hh).view(1, 1, hh, 1).float(), torch.arange(ww).view(1, 1, 1, ww).float()
    tgt = torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / 18.0)
    tw = (torch.rand(B, 17, 1, generator=g) < 0.8).float()
    return img, tgt, tw


def test_eval_is_batch_independent_at_full_size():
    """Eval-mode output of sample i must not depend on the batch it sits in: the B=32 plan
    (other tile shapes, 16x more virtual rows) must reproduce the B=2 plan exactly."""
    torch.manual_seed(1)
    m = PoseHighResolutionNet("w32", "bf16").cuda().eval()
    img, _, _ = _batch(32, 384, 288)
    with torch.no_grad():
        big = m(img.cuda())
        small = m(img[:2].cuda())
        last = m(img[30:].cuda())
    assert big.shape == (32, 17, 96, 72)
    assert torch.equal(big[:2], small)
    assert torch.equal(big[30:], last)
    assert torch.isfinite(big).all()


def test_fused_train_step_full_size_loss_decreases():
    torch.manual_seed(2)
    m = PoseHighResolutionNet("w32", "bf16").cuda()
    ts = TrainStep(m, 32, 384, 288, optimizer="adam", lr=1e-3)
    img, tgt, tw = _batch(32, 384, 288, seed=3)
    ts.load_batch(img.cuda(), tgt.cuda(), tw.cuda())
    losses = [float(ts.step().item()) for _ in range(6)]
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < 0.7 * losses[0], losses
    assert int(ts.step_count.item()) == 6
    # BN bookkeeping follows the reference module: one num_batches_tracked increment per forward
    assert int(m.bn1.num_batches_tracked.item()) == 6
    # the drop-in autograd path on the same weights gives the same loss as the fused step would
    from stlpose_amd import PersonMSELoss
    out = m(img.cuda())
    l2 = PersonMSELoss()(out, tgt.cuda(), tw.cuda())
    l2.backward()
    assert abs(l2.item() - float(ts.step().item())) < 0.05 * abs(l2.item()) + 1e-4
    assert m.final_layer.weight.grad is not None and torch.isfinite(m.final_layer.weight.grad).all()


def test_sgd_nesterov_step_runs():
    torch.manual_seed(4)
    m = PoseHighResolutionNet("tiny", "fp32").cuda()
    ts = TrainStep(m, 2, 64, 64, optimizer="sgd", lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4)  # model_setup.py:139-141
    img, tgt, tw = _batch(2, 64, 64, seed=5)
    ts.load_batch(img.cuda(), tgt.cuda(), tw.cuda())
    l0 = float(ts.step().item())
    for _ in range(10):
        l = float(ts.step().item())
    assert np.isfinite(l) and l < l0


def test_gradient_buckets_cover_the_flat_buffer_and_dp_path_matches(monkeypatch):
    """The backward program reduces the weight-gradient slabs bucket by bucket (no serial tail) and
    records an event per bucket; the data-parallel path all-reduces each bucket on a communication
    stream as soon as that event fires.  With ONE rank (RCCL all-reduce = identity) the bucketed path
    must give exactly the gradients and losses of the plain path."""
    import torch.distributed as dist
    torch.manual_seed(5)
    img, tgt, tw = _batch(4, 256, 192, seed=7)

    def run(dp):
        torch.manual_seed(11)
        m = PoseHighResolutionNet("w32", "bf16").cuda()
        pg = None
        if dp:
            if not dist.is_initialized():
                dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29577", rank=0, world_size=1)
            pg = dist.group.WORLD
            monkeypatch.setenv("STLPOSE_DP_FORCE", "1")
        ts = TrainStep(m, 4, 256, 192, optimizer="sgd", lr=1e-2, process_group=pg)
        ts.load_batch(img.cuda(), tgt.cuda(), tw.cuda())
        losses = [float(ts.step().item()) for _ in range(3)]
        torch.cuda.synchronize()
        return ts, losses, ts.store.grads.clone(), ts.store.master.clone()

    ts0, l0, g0, w0 = run(False)
    bk = ts0.eng.buckets
    assert len(bk) >= 3
    # buckets tile the flat parameter buffer from the back (last layers first), without gaps
    assert bk[0]["hi"] == ts0.store.nparam and bk[-1]["lo"] == 0
    assert all(bk[i]["lo"] == bk[i + 1]["hi"] for i in range(len(bk) - 1))
    ts1, l1, g1, w1 = run(True)
    assert ts1.dp is not None and len(ts1.dp.buckets) == len(bk)
    assert l0 == l1
    assert torch.equal(g0, g1) and torch.equal(w0, w1)
    if dist.is_initialized():
        dist.destroy_process_group()


def test_bf16_gradient_buckets_on_a_one_rank_rccl_group(monkeypatch):
    """bf16 gradient buckets through the real overlapped path on a one-rank RCCL communicator: the
    collective moves bf16 copies, the fp32 gradient buffer receives them back -- every gradient within bf16 rounding
    (2^-8 of its own magnitude) of the fp32-bucket run, the optimiser's factor is 1 (the buckets carry the mean)."""
    import torch.distributed as dist
    monkeypatch.setenv("STLPOSE_DP_FORCE", "1")
    img, tgt, tw = _batch(4, 256, 192, seed=7)
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29578", rank=0, world_size=1)
    try:
        res = []
        for bf16 in (False, True):
            torch.manual_seed(11)
            m = PoseHighResolutionNet("w32", "bf16").cuda()
            ts = TrainStep(m, 4, 256, 192, optimizer="sgd", lr=0.0, momentum=0.0, process_group=dist.group.WORLD, bf16_buckets=bf16)
            ts.load_batch(img.cuda(), tgt.cuda(), tw.cuda())
            ts.step()
            torch.cuda.synchronize()
            res.append((ts.store.grads.clone(), float(ts.hyper[7].item()), ts.dp.bf16))
        (g32, s32, b32), (g16, s16, b16) = res
        assert (b32, b16) == (False, True) and s32 == 1.0 and s16 == 1.0     # world 1: 1 / world = 1 either way
        assert not torch.equal(g32, g16)                                      # the bf16 round trip did happen
        assert float(((g16 - g32).abs() - g32.abs() * 2.0 ** -8).max()) <= 1e-12
    finally:
        dist.destroy_process_group()


def test_backward_stream_layouts_give_the_same_gradients(monkeypatch):
    """The planner's stream layouts (four streams with the off-chain launches list-scheduled onto idle branch streams =
    default, two streams, one stream; grouped or single weight gradients) only move launches between queues: losses
    identical, gradients identical up to the order of the fp64 statistics atomics."""
    img, tgt, tw = _batch(4, 256, 192, seed=13)

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        torch.manual_seed(17)
        m = PoseHighResolutionNet("w32", "fp32").cuda()
        ts = TrainStep(m, 4, 256, 192, optimizer="sgd", lr=0.0, momentum=0.0)
        ts.load_batch(img.cuda(), tgt.cuda(), tw.cuda())
        l = float(ts.step().item())
        torch.cuda.synchronize()
        g = ts.store.grads.clone()
        n = ts.eng.nstreams
        for k in env:
            monkeypatch.delenv(k)
        return l, g, n
    l0, g0, n0 = run({})
    assert n0 == 4
    for env, nstreams in (({"STLPOSE_STREAMS": "2"}, 2), ({"STLPOSE_STREAMS": "1"}, 1), ({"STLPOSE_WGRAD_GROUP": "1"}, 4)):
        l1, g1, n1 = run(env)
        assert n1 == nstreams, (env, n1)
        assert l1 == l0, env
        assert float((g1 - g0).abs().max()) <= 1e-5 * float(g0.abs().max()), env
