"""CPU: the C ABI and op of the any-N full ranking (stl_pose_rank_any) refuse bad arguments before any device work."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from stlpose_amd import build, capi
    build.build(verbose=False)
    return capi.lib()


def _rank_any(L, n, k_out=0, idx=None, dist=None, labels=None, qlabels=None, nl=0, k_eff=0, scores=None, q=None, db=None, work=None,
              work_bytes=0):
    return L.stl_pose_rank_any(q, None, db, 1, n, 26, 0, 0, k_out, idx, dist, labels, qlabels, nl, k_eff, scores, work, work_bytes, None)


def test_symbols_exist(L):
    from stlpose_amd import capi
    assert hasattr(L, "stl_pose_rank_any") and hasattr(L, "stl_pose_rank_any_workspace")
    assert L.stl_pose_rank_any_workspace.restype is C.c_int64
    assert capi.POSE_RANK_ANY_MAX == 1 << 24 and capi.POSE_RANK_MAX == 16384


def test_workspace_size(L):
    ws = L.stl_pose_rank_any_workspace
    assert ws(1, 1) > 0 and ws(1, 16384) > 0 and ws(0, 20000) > 0
    assert 0 < ws(1, 16385) < ws(2, 16385) < ws(2, 16386) < ws(2, 40000) < ws(5, 40000)
    assert ws(1, 16385) >= 2 * 8 * 16385                      # two arrays of 8-byte keys
    assert ws(65535, 1 << 24) > 1 << 40                        # no 32-bit overflow at the largest call
    for n in (0, -1, (1 << 24) + 1):
        assert ws(1, n) < 0 and b"16777216" in L.stl_last_error()
    assert ws(-1, 100) < 0
    assert ws(1, 1 << 24) > 0


def test_rank_any_refuses_bad_arguments(L):
    # N = 16385 is accepted: with null pointers the call fails on the pointer check
    assert _rank_any(L, 16385) < 0
    assert b"null pointer" in L.stl_last_error() and b"N =" not in L.stl_last_error()
    assert _rank_any(L, (1 << 24) + 1) < 0 and b"16777216" in L.stl_last_error()
    assert _rank_any(L, 0) < 0 and b"16777216" in L.stl_last_error()
    assert _rank_any(L, 20000, k_out=20001) < 0 and b"k_out" in L.stl_last_error()
    lab = (C.c_int32 * 20000)()
    assert _rank_any(L, 20000, labels=lab, qlabels=lab, nl=1, k_eff=10, scores=lab) < 0 and b"k_eff" in L.stl_last_error()
    assert _rank_any(L, 20000, labels=lab, qlabels=lab, nl=1, k_eff=20001, scores=lab) < 0 and b"k_eff" in L.stl_last_error()
    assert _rank_any(L, 20000, labels=lab, qlabels=None, nl=1, k_eff=20, scores=lab) < 0 and b"qlabels" in L.stl_last_error()
    assert _rank_any(L, 20000, labels=lab, qlabels=lab, nl=5, k_eff=20, scores=lab) < 0 and b"L <=" in L.stl_last_error()
    assert L.stl_pose_rank_any(None, None, None, 1, 20000, 20, 0, 0, 0, None, None, None, None, 0, 0, None, None, 0, None) < 0
    assert b"D = 20" in L.stl_last_error()
    assert L.stl_pose_rank_any(None, None, None, 1, 20000, 26, 9, 0, 0, None, None, None, None, 0, 0, None, None, 0, None) < 0
    assert b"method" in L.stl_last_error()


def test_rank_any_refuses_a_short_workspace(L):
    """Host buffers stand in for device memory: the workspace check comes before any launch, so they are never touched."""
    buf = (C.c_float * 64)()
    need = L.stl_pose_rank_any_workspace(1, 20000)
    for work, nbytes in ((buf, need - 1), (buf, 0), (None, need)):
        assert _rank_any(L, 20000, q=buf, db=buf, work=work, work_bytes=nbytes) < 0
        assert b"workspace" in L.stl_last_error() and str(need).encode() in L.stl_last_error()
    assert _rank_any(L, 1000, q=buf, db=buf, work=None, work_bytes=0) < 0 and b"workspace" in L.stl_last_error()


def test_pose_rank_keeps_its_limit(L):
    assert L.stl_pose_rank(None, None, None, 1, 16385, 26, 0, 0, 0, None, None, None, None, 0, 0, None, None) < 0
    assert b"16384" in L.stl_last_error()


def test_op_registered_with_fake():
    import torch
    import stlpose_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.stlpose, "pose_rank_any")
    schema = torch.ops.stlpose.pose_rank_any.default._schema
    assert [a.name for a in schema.arguments] == [a.name for a in torch.ops.stlpose.pose_rank.default._schema.arguments]
    with FakeTensorMode():
        q, db = torch.empty(3, 34), torch.empty(40000, 34)
        lab, qlab = torch.empty(2, 40000, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        idx, dist, s = torch.ops.stlpose.pose_rank_any(q, None, db, "euclidean", "none", 1025, lab, qlab, 40000)
        assert idx.shape == (3, 1025) and idx.dtype == torch.int64
        assert dist.shape == (3, 1025) and dist.dtype == torch.float32
        assert s.shape == (3, 2, 10) and s.dtype == torch.float64
        idx, dist, s = torch.ops.stlpose.pose_rank_any(q, None, db, "euclidean", "none", 0, None, None, 0)
        assert idx.shape == (3, 0) and dist.shape == (3, 0) and s.shape == (3, 0, 10)


def test_shape_mismatches_raise_before_any_launch():
    import torch
    from stlpose_amd import ops
    q34, q26, db26 = torch.zeros(3, 34), torch.zeros(3, 26), torch.zeros(50, 26)
    lab = torch.zeros(2, 50, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="width"):
        ops._pose_rank_any(q34, None, db26, "euclidean", "none", 5, None, None, 0)
    with pytest.raises(RuntimeError, match="labels"):
        ops._pose_rank_any(q26, None, db26, "euclidean", "none", 0, torch.zeros(2, 49, dtype=torch.int32), lab[:, :3], 20)
    with pytest.raises(RuntimeError, match="qlabels"):
        ops._pose_rank_any(q26, None, db26, "euclidean", "none", 0, lab, None, 20)
