"""CPU: the planner's ``input_grad`` plans (dry run, no kernel is launched): the plans without the flag are untouched, the
training plan adds exactly the stem's data gradient and one ``stl_patch3x3_backward``, the eval plan is a data-gradient-only
backward whose BatchNorm-backward sources read the running statistics and a zero ``rstats`` arena and whose reductions all
land in the sink arena."""
import ctypes as C
from collections import Counter

import pytest
import torch

from stlpose_amd import PoseHighResolutionNet, capi
from stlpose_amd.engine import Engine


def _fields(desc):
    """Every scalar field of a descriptor (recursively); pointers only as null / non-null (buffers differ between plans)."""
    out = []
    for name, typ in desc._fields_:
        v = getattr(desc, name)
        if isinstance(v, C.Structure):
            out.append((name, _fields(v)))
        elif isinstance(v, C.Array):
            out.append((name, tuple(_fields(e) if isinstance(e, C.Structure) else bool(e) for e in v)))
        elif typ is C.c_void_p:
            out.append((name, v is not None))
        else:
            out.append((name, v))
    return tuple(out)


def _ops(ops):
    return [(o[0], o[2], _fields(o[1]) if isinstance(o[1], C.Structure) else None) for o in ops]


@pytest.fixture(scope="module")
def model():
    m = PoseHighResolutionNet("w32", "fp32")
    m._pack(torch.device("cpu"))
    return m


@pytest.mark.parametrize("dt", [capi.F32, capi.MIXED])
def test_training_plan_with_input_grad_adds_stem_dgrad_and_patch_backward(model, dt):
    a = Engine(model.arch, model._store, 2, 128, 96, dt, True)
    b = Engine(model.arch, model._store, 2, 128, 96, dt, True, input_grad=True)
    assert a.dimg is None and b.dimg is not None and tuple(b.dimg.shape) == (2, 3, 128, 96)
    assert _ops(a.fwd_ops) == _ops(b.fwd_ops)
    # backward: the same ops in the same order (streams aside: the list scheduler sees two more launches), plus exactly two
    fa = [(n, f) for n, _, f in _ops(a.bwd_ops)]
    fb = [(n, f) for n, _, f in _ops(b.bwd_ops)]
    extra = Counter(n for n, _ in fb) - Counter(n for n, _ in fa)
    assert extra == Counter({"stl_conv_forward": 1, "stl_patch3x3_backward": 1})
    dg = [o for o in b.bwd_ops if o[0] == "stl_conv_forward" and o[1].Co == 32 and o[1].ks == 1 and o[1].Hi == 64 and o[1].Ci == 64]
    assert len(dg) == 1
    d = dg[0][1]
    assert d.src.mode == capi.SRC_BNBWD and not d.mask_y and not d.red and not d.addend and d.stuff == 0
    assert d.w == b.wk.data_ptr() + b.convs[0].bwd_off * b.esz
    pb = [o for o in b.bwd_ops if o[0] == "stl_patch3x3_backward"]
    assert len(pb) == 1 and pb[0][3] == [d.out] and pb[0][4] == [b.dimg.data_ptr()]
    assert pb[0][1].stride == 2 and pb[0][1].dtype == (dt & 0xff) and pb[0][1].dimg == b.dimg.data_ptr()
    assert b.bwd_ops.index(pb[0]) > b.bwd_ops.index(dg[0])
    rest = [x for x in fb if x[1] is not None and x != ("stl_conv_forward", _fields(d))]
    rest = [x for x in rest if x[0] != "stl_patch3x3_backward"]
    assert rest == fa
    # weight layouts: only the patch conv gains a data-gradient layout
    assert a.convs[0].bwd_off == -1 and b.convs[0].bwd_off >= 0
    assert [c.bwd_off >= 0 for c in a.convs[1:]] == [c.bwd_off >= 0 for c in b.convs[1:]]
    assert len(a.slabs) == len(b.slabs) and len(a.buckets) == len(b.buckets)


def test_plans_without_input_grad_are_unchanged(model):
    """The flag's default is off, and a plan without it has no image gradient, a patch tensor without a data gradient and
    (eval) no backward program at all."""
    for training in (True, False):
        e = Engine(model.arch, model._store, 2, 64, 64, capi.BF16, training)
        assert not e.input_grad and e.dimg is None and e.sink is None
        assert e.convs[0].bwd_off == -1
        assert "stl_patch3x3_backward" not in {o[0] for o in e.bwd_ops}
        e2 = Engine(model.arch, model._store, 2, 64, 64, capi.BF16, training, input_grad=False)
        assert _ops(e.fwd_ops) == _ops(e2.fwd_ops) and _ops(e.bwd_ops) == _ops(e2.bwd_ops)
    assert not Engine(model.arch, model._store, 2, 64, 64, capi.BF16, False).bwd_ops


@pytest.mark.parametrize("dt", [capi.F32, capi.MIXED])
def test_eval_plan_with_input_grad_is_data_gradient_only(model, dt):
    a = Engine(model.arch, model._store, 2, 128, 96, dt, False)
    e = Engine(model.arch, model._store, 2, 128, 96, dt, False, input_grad=True)
    assert _ops(a.fwd_ops) == _ops(e.fwd_ops)   # the eval forward itself is unchanged
    names = Counter(o[0] for o in e.bwd_ops)
    assert set(names) == {"stl_conv_forward", "stl_fuse_backward", "stl_upsample_backward", "stl_head_backward",
                          "stl_patch3x3_backward"}
    assert names["stl_patch3x3_backward"] == 1 and names["stl_head_backward"] == 1
    assert names["stl_conv_forward"] == 292 and names["stl_upsample_backward"] == 28   # every conv's data gradient, incl. the stem's
    assert not e.slabs and not e.buckets
    nst = e.rstats.numel() * 8
    zero = (e.rstats.data_ptr(), e.rstats.data_ptr() + nst)
    sink = (e.sink.data_ptr(), e.sink.data_ptr() + nst)

    def inside(p, r):
        return p is not None and r[0] <= p < r[1]

    def bnbwd_ok(s):   # running statistics, zero rstats
        return s.stats is None and s.rmean is not None and s.rvar is not None and inside(s.rstats, zero)

    for name, d, _, _, _ in e.bwd_ops:
        if name == "stl_conv_forward":
            assert d.src.mode == capi.SRC_BNBWD and bnbwd_ok(d.src)
            assert d.out_stats is None
            if d.mask_y:
                assert d.mask_bn.stats is None and d.mask_bn.rmean is not None   # ReLU masks of the eval-mode BN
            if d.red:
                assert inside(d.red, sink)
        elif name == "stl_fuse_backward":
            for i in range(d.nbn):
                assert d.bn[i].stats is None and d.bn[i].rmean is not None and inside(d.rstats[i], sink)
        elif name == "stl_upsample_backward":
            assert d.bn.stats is None and d.bn.rmean is not None and inside(d.rstats, sink)
    # the BNADD block ends of the eval forward store the sum that backward reads as z
    for o in e.fwd_ops:
        if o[0] == "stl_conv_forward" and o[1].src.mode == capi.SRC_BNADD:
            assert o[1].src_out
    assert e.convs[0].bwd_off >= 0 and all(c.bwd_off >= 0 for c in e.convs)


def test_module_plan_key_carries_input_grad():
    m = PoseHighResolutionNet("tiny", "fp32")
    m._pack(torch.device("cpu"))
    plain, grad = m.engine(2, 64, 64, True), m.engine(2, 64, 64, True, True)
    assert plain is not grad and not plain.input_grad and grad.input_grad
    assert m.engine(2, 64, 64, True, False) is plain
    ev = m.engine(2, 64, 64, False, True)
    assert ev.input_grad and not ev.training and ev.bwd_ops
