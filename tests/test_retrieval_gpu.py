"""GPU: pose retrieval kernels (csrc/retrieval.hip) against the reference's own outputs (tests/golden/retrieval/g13_retrieval.npz)
and against themselves (top-k / rank == a stable argsort of pose_distances, bit for bit)."""
import os

import numpy as np
import pytest
import torch

from tests import retrieval_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "retrieval", "g13_retrieval.npz")
REF_METHODS = {"euclidean_distance": "euclidean", "cosine_similarity": "cosine", "manhattan_distance": "manhattan",
               "confidence_score": "confidence", "oks_score": "oks"}
PENS = ("zero_coord", "none", "mean", "max")
KEYS = ("p@1", "p@5", "p@10", "p@rel", "mAP", "r@1", "r@5", "r@10", "r@rel", "mAR")


@pytest.fixture(scope="module")
def g():
    import stlpose_amd  # noqa: F401
    return np.load(FIX)


def _cuda(x, dt=torch.float32):
    return torch.as_tensor(np.asarray(x)).to("cuda", dt).contiguous()


def _conf(m, g):
    return _cuda(g["conf"]) if m == "confidence_score" else None


def test_pose_vectors_match_reference(g):
    for ap in ("all_kpts", "full_body", "upper_body"):
        for norm in (1, 0):
            want = g[f"vec_{ap}_{norm}"]
            got = torch.ops.stlpose.pose_vectors(_cuda(g["joints_db"]), ap, bool(norm)).cpu().numpy()
            assert got.shape == want.shape
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
            assert np.array_equal(got == 0, want == 0), (ap, norm)
    # strided joints (row stride > 17 * C) and the single-vector drop-in
    from stlpose_amd import process_pose_vector
    big = np.zeros((300, 20, 4), np.float32)
    big[:, :17, :3] = g["joints_db"]
    got = torch.ops.stlpose.pose_vectors(_cuda(big)[:, :17, :], "full_body", True).cpu().numpy()
    np.testing.assert_allclose(got, g["vec_full_body_1"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(process_pose_vector(g["joints_q"][0], "full_body"), g["q"][0], rtol=0, atol=1e-6)


def _ref_dist_rows(g, m, p):
    c = g["conf"] if m == "confidence_score" else [None] * len(g["q"])
    return np.stack([R.distances(REF_METHODS[m], p, g["q"][i], g["db"], c[i]) for i in range(len(g["q"]))])


def test_pose_distances_match_reference(g):
    n = g["db"].shape[0]
    for m in REF_METHODS:
        for p in PENS:
            got = torch.ops.stlpose.pose_distances(_cuda(g["q"]), _conf(m, g), _cuda(g["db"]), REF_METHODS[m], p).cpu().numpy()
            full = g[f"dist_{m}_{p}_{n}"]   # the reference's distances, in its ranked order
            want = np.empty_like(full)
            np.put_along_axis(want, g[f"idx_{m}_{p}_{n}"], full, axis=1)
            scale = np.nanmax(np.abs(want), axis=1, keepdims=True)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (m, p)
            assert np.nanmax(np.abs(got - want) / scale) <= 1e-5, (m, p)


def _stable(d):
    idx = np.argsort(d, axis=1, kind="stable")
    return idx, np.take_along_axis(d, idx, axis=1)


def _check_exact(q, conf, db, method, pen, ks, rank=True):
    d = torch.ops.stlpose.pose_distances(q, conf, db, method, pen).cpu().numpy()
    idx_all, dist_all = _stable(d)
    for k in ks:
        if k > db.shape[0]:
            continue
        if k <= 1024:
            i, v = torch.ops.stlpose.pose_topk(q, conf, db, method, pen, k)
            assert np.array_equal(i.cpu().numpy(), idx_all[:, :k]), (method, pen, k, db.shape[0], q.shape[0])
            assert np.array_equal(v.cpu().numpy().view(np.uint32), dist_all[:, :k].view(np.uint32)), (method, pen, k)
    if rank and db.shape[0] <= 16384:
        i, v, _ = torch.ops.stlpose.pose_rank(q, conf, db, method, pen, db.shape[0], None, None, 0)
        assert np.array_equal(i.cpu().numpy(), idx_all), (method, pen, db.shape[0])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), dist_all.view(np.uint32))


def test_topk_and_rank_equal_stable_argsort_of_distances():
    gen = torch.Generator(device="cuda").manual_seed(0)
    ks = (1, 10, 11, 100, 1024)
    for n in (1, 63, 64, 65, 1000, 16384):
        db = torch.rand(n, 26, device="cuda", generator=gen)
        db[: n // 3] = torch.round(db[: n // 3] * 4) / 4   # coarse values: many exact distance ties
        if n > 2:
            db[n // 2] = db[1]                                # exact duplicate rows
        for nq in (1, 7):
            q = torch.rand(nq, 26, device="cuda", generator=gen)
            q[:, 4] = 0
            _check_exact(q, None, db, "euclidean", "none", ks)
            _check_exact(q, None, db, "manhattan", "mean", (10,), rank=n <= 1000)
    db = torch.rand(1000, 26, device="cuda", generator=gen)
    q = torch.rand(4096, 26, device="cuda", generator=gen)
    _check_exact(q, None, db, "cosine", "zero_coord", (1, 11, 100))
    conf = torch.rand(7, 34, device="cuda", generator=gen)
    conf[2] = 0                                              # all-zero confidence: every distance NaN, sorted by index
    dbc, qc = torch.rand(1000, 34, device="cuda", generator=gen), torch.rand(7, 34, device="cuda", generator=gen)
    _check_exact(qc, conf, dbc, "confidence", "max", ks)
    _check_exact(qc, None, dbc, "oks", "none", (10, 100))
    dbl = torch.rand(100003, 18, device="cuda", generator=gen)
    dbl[777] = dbl[99999]
    _check_exact(torch.rand(7, 18, device="cuda", generator=gen), None, dbl, "l2sq", "zero_coord", ks, rank=False)
    _check_exact(torch.rand(1, 18, device="cuda", generator=gen), None, dbl, "euclidean", "max", (1, 100, 1024), rank=False)


def _check_against_reference(idx, dist, g, m, p, k):
    """distances within tolerance; the reference distance of our r-th index within tolerance of its r-th distance."""
    n = g["db"].shape[0]
    full = g[f"dist_{m}_{p}_{n}"]
    ref_rows = np.empty_like(full)
    np.put_along_axis(ref_rows, g[f"idx_{m}_{p}_{n}"], full, axis=1)
    want = g[f"dist_{m}_{p}_{k}"]
    scale = np.nanmax(np.abs(ref_rows), axis=1, keepdims=True)
    assert idx.shape == want.shape
    tol = 1e-5 * scale
    assert np.all((np.abs(dist - want) <= tol) | (np.isnan(dist) & np.isnan(want))), (m, p, k)
    mine = np.take_along_axis(ref_rows, idx, axis=1)
    assert np.all((np.abs(mine - want) <= tol) | (np.isnan(mine) & np.isnan(want))), (m, p, k)


def test_topk_and_rank_match_reference_rankings(g):
    n = g["db"].shape[0]
    for m in REF_METHODS:
        for p in PENS:
            for k in (12, n):
                if k <= 1024:
                    i, v = torch.ops.stlpose.pose_topk(_cuda(g["q"]), _conf(m, g), _cuda(g["db"]), REF_METHODS[m], p, k)
                    _check_against_reference(i.cpu().numpy(), v.cpu().numpy(), g, m, p, k)
                i, v, _ = torch.ops.stlpose.pose_rank(_cuda(g["q"]), _conf(m, g), _cuda(g["db"]), REF_METHODS[m], p, k, None, None, 0)
                _check_against_reference(i.cpu().numpy(), v.cpu().numpy(), g, m, p, k)


def test_rank_scores_equal_host_scoring(g):
    from stlpose_amd.retrieval import score_retrievals
    rng = np.random.default_rng(3)
    n = 2000
    db = _cuda(rng.uniform(size=(n, 26)))
    lab = np.stack([rng.integers(0, 40, n), rng.integers(0, 6, n)]).astype(np.int32)
    lab[0, 5] = 999                                           # a label no other pose has: scores -1
    for nl in (1, 2):
        for k_eff in (n, 50):
            idx, _, s = torch.ops.stlpose.pose_rank(db, None, db, "euclidean", "zero_coord", n, _cuda(lab[:nl], torch.int32),
                                                    _cuda(lab[:nl], torch.int32), k_eff)
            idx, s = idx.cpu().numpy(), s.cpu().numpy()
            for qi in range(0, n, 37):
                for li in range(nl):
                    h = score_retrievals(int(lab[li, qi]), list(lab[li, idx[qi, :k_eff]]))
                    np.testing.assert_allclose(s[qi, li], [h[k] for k in KEYS], rtol=0, atol=1e-12)
            assert np.all(s[5, 0] == -1)
    # the fixture's label lists as rankings: a database whose row j carries label row[j], each query at distance 0 from row 0
    for row, want in zip(g["score_labels"], g["score_values"]):
        m = len(row)
        dbv = np.zeros((m, 18), np.float32)
        dbv[:, 0] = np.arange(m, dtype=np.float32)
        _, _, s = torch.ops.stlpose.pose_rank(_cuda(dbv[:1]), None, _cuda(dbv), "euclidean", "zero_coord", 0,
                                              _cuda(row[None], torch.int32), _cuda(row[:1][None], torch.int32), m)
        np.testing.assert_allclose(s.cpu().numpy()[0, 0], want, rtol=0, atol=1e-12)


def test_get_neighbors_idxs_drop_in(g):
    from stlpose_amd import PoseIndex, get_neighbors_idxs
    n = g["db"].shape[0]
    for m in REF_METHODS:
        for p in PENS:
            for k in (12, n):
                ii, dd = [], []
                for qi in range(len(g["q"])):
                    kw = {"scores": g["conf"][qi]} if m == "confidence_score" else {}
                    i, d = get_neighbors_idxs(g["q"][qi], num_retrievals=k, approach="full_body", retrieval_method=m, penalization=p,
                                              database=g["db"], **kw)
                    ii.append(i), dd.append(d)
                _check_against_reference(np.stack(ii), np.stack(dd), g, m, p, k)
    ib, db_ = get_neighbors_idxs(g["q"], num_retrievals=12, retrieval_method="euclidean_distance", penalization="none", database=g["db"])
    _check_against_reference(ib, db_, g, "euclidean_distance", "none", 12)
    index = PoseIndex(space="l2", dim=26)
    index.init_index(max_elements=n, ef_construction=1000, M=8)
    index.add_items(g["db"], np.arange(n))
    i, d = get_neighbors_idxs(g["q"][0], num_retrievals=12, retrieval_method="knn", knn=index)
    want = np.sum((g["db"].astype(np.float64) - g["q"][0]) ** 2, axis=1)
    assert i.shape == (12,) and np.array_equal(i.astype(np.int64), np.argsort(want, kind="stable")[:12])
    np.testing.assert_allclose(d, want[i.astype(np.int64)], rtol=1e-5, atol=1e-6)


def test_pose_index(tmp_path):
    from stlpose_amd import PoseIndex
    rng = np.random.default_rng(7)
    data, q = rng.normal(size=(3000, 34)).astype(np.float32), rng.normal(size=(5, 34)).astype(np.float32)
    ids = np.arange(3000, dtype=np.uint64) * 7 + (1 << 40)
    for space in ("l2", "cosine"):
        index = PoseIndex(space=space, dim=34)
        index.init_index(max_elements=3000)
        index.set_ef(50)
        index.add_items(data[:1000], ids[:1000])
        index.add_items(data[1000:], ids[1000:])
        assert index.get_current_count() == 3000
        lab, dist = index.knn_query(q, k=20)
        assert lab.dtype == np.uint64 and dist.dtype == np.float32 and lab.shape == (5, 20)
        x, y = data.astype(np.float64), q.astype(np.float64)
        if space == "l2":
            full = ((y[:, None, :] - x[None]) ** 2).sum(-1)
        else:
            full = 1 - (y / np.linalg.norm(y, axis=1, keepdims=True)) @ (x / np.linalg.norm(x, axis=1, keepdims=True)).T
        order = np.argsort(full, axis=1, kind="stable")[:, :20]
        assert np.array_equal(lab, ids[order])
        np.testing.assert_allclose(dist, np.take_along_axis(full, order, 1), rtol=1e-5, atol=1e-5)
        path = os.path.join(str(tmp_path), f"graph_{space}.pkl")
        index.save_index(path)
        assert os.path.exists(path)
        back = PoseIndex(space=space, dim=34)
        back.load_index(path, max_elements=0)
        l2, d2 = back.knn_query(q, k=20)
        assert np.array_equal(l2, lab) and np.array_equal(d2, dist)
        with pytest.raises(RuntimeError):
            back.knn_query(q, k=3001)


def test_retrieval_experiment_end_to_end():
    from stlpose_amd import retrieval_experiment
    rng = np.random.default_rng(11)
    n = 2000
    # values on a 1/8 grid: every distance below is exact in fp32 and fp64, so both sides see the same order (ties by index)
    feats = (rng.integers(-8, 9, (n, 26)) / 8).astype(np.float32)
    chars = [f"c{v}" for v in rng.integers(0, 30, n)]
    narr = [f"n{int(c[1:]) % 5}" for c in chars]
    for method, pen in (("euclidean_distance", "zero_coord"), ("manhattan_distance", "none")):
        res = retrieval_experiment(feats, {"character": chars, "narrative": narr}, "full_body", method, pen, num_retrievals=-1)
        d = np.stack([R.distances(REF_METHODS[method], pen, feats[i], feats) for i in range(0, n, 97)])
        for row, qi in enumerate(range(0, n, 97)):
            order = np.argsort(d[row], kind="stable")
            for level, labs in (("character", chars), ("narrative", narr)):
                want = R.score([labs[qi]][0], [labs[j] for j in order])
                got = res[level][qi]
                assert got["label"] == labs[qi]
                np.testing.assert_allclose([got[k] for k in KEYS], want, rtol=0, atol=1e-9, err_msg=f"{method} {level} {qi}")
    with pytest.raises(NotImplementedError):
        torch.ops.stlpose.pose_topk(torch.zeros(2, 26), None, torch.zeros(20, 26), "euclidean", "none", 3)


def test_width_mismatch_raises_on_device_tensors():
    """A 34-wide all_kpts query against a 26-wide database (or index) is refused before the kernel would read past the rows."""
    from stlpose_amd import PoseIndex, get_neighbors_idxs
    q, db = torch.rand(2, 34, device="cuda"), torch.rand(1000, 26, device="cuda")
    with pytest.raises(RuntimeError, match="width"):
        torch.ops.stlpose.pose_topk(q, None, db, "euclidean", "none", 10)
    with pytest.raises(RuntimeError, match="width"):
        get_neighbors_idxs(np.zeros(34, np.float32), 10, retrieval_method="euclidean_distance", penalization="none",
                           database=np.zeros((1000, 26), np.float32))
    index = PoseIndex(space="l2", dim=26)
    index.init_index(max_elements=1000)
    index.add_items(db.cpu().numpy())
    with pytest.raises(RuntimeError, match="dimensionality"):
        index.knn_query(q.cpu().numpy(), k=5)
    torch.cuda.synchronize()
