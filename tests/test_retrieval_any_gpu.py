"""GPU: the full ranking above N = 16384 (stlpose::pose_rank_any: sorted runs, merge path, scores from global memory) against a
stable argsort of pose_distances (bit for bit), the existing kernels, host scoring of its own ranking, and through the public
interface (retrieval_experiment, search / get_neighbors_idxs / PoseIndex).

Sizes: 16385 = two runs, the second of one key; 32768 = two full runs; 40000 = three runs, so the first merge pass copies an odd
run; 100003 = seven runs, three passes over unequal runs.  16384 and 1000 take the single-workgroup kernel."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("p@1", "p@5", "p@10", "p@rel", "mAP", "r@1", "r@5", "r@10", "r@rel", "mAR")
COUNT_COLS, MEAN_COLS = [0, 1, 2, 3, 5, 6, 7, 8], [4, 9]
COMBOS = (("euclidean", "none"), ("manhattan", "mean"), ("cosine", "zero_coord"), ("confidence", "max"), ("oks", "none"))


def _cuda(x, dt=torch.float32):
    return torch.as_tensor(np.asarray(x)).to("cuda", dt).contiguous()


@functools.lru_cache(maxsize=None)
def _data(n, nq, d):
    """(db [n, d], q [nq, d], conf [nq, d]) on the GPU: a third of the rows on a 1/4 grid (many exact distance ties), one row
    repeated in different runs, a zero coordinate in every query (the mean / max penalty applies), and, from three queries up,
    one all-zero confidence (every distance NaN: ordered by index)."""
    import stlpose_amd  # noqa: F401
    rng = np.random.default_rng(n * 131 + nq * 7 + d)
    db = rng.uniform(size=(n, d)).astype(np.float32)
    db[: n // 3] = np.round(db[: n // 3] * 4) / 4
    if n > 16384:
        db[16384] = db[1]
    db[n - 1] = db[1]
    q = rng.uniform(size=(nq, d)).astype(np.float32)
    q[:, 4] = 0
    conf = rng.uniform(size=(nq, d)).astype(np.float32)
    if nq >= 3:
        conf[2] = 0
    return _cuda(db), _cuda(q), _cuda(conf)


@functools.lru_cache(maxsize=None)
def _stable(n, nq, d, method, pen):
    """The yardstick, computed once per case: (idx, dist) of a stable argsort of pose_distances."""
    db, q, conf = _data(n, nq, d)
    dd = torch.ops.stlpose.pose_distances(q, conf if method == "confidence" else None, db, method, pen).cpu().numpy()
    idx = np.argsort(dd, axis=1, kind="stable")
    return idx, np.take_along_axis(dd, idx, axis=1)


def _rank_any(n, nq, d, method, pen, k_out, labels=None, qlabels=None, k_eff=0):
    db, q, conf = _data(n, nq, d)
    i, v, s = torch.ops.stlpose.pose_rank_any(q, conf if method == "confidence" else None, db, method, pen, k_out, labels, qlabels, k_eff)
    return i.cpu().numpy(), v.cpu().numpy(), s.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("d", (18, 34))
@pytest.mark.parametrize("nq", (1, 5))
@pytest.mark.parametrize("n", (16385, 32768, 40000))
def test_ranking_equals_stable_argsort_bit_for_bit(n, nq, d):
    for method, pen in COMBOS:
        idx_all, dist_all = _stable(n, nq, d, method, pen)
        for k in (n, 0, 1, 1025):
            i, v, s = _rank_any(n, nq, d, method, pen, k)
            assert i.shape == (nq, k) and v.shape == (nq, k) and s.shape == (nq, 0, 10)
            assert np.array_equal(i, idx_all[:, :k]), (method, pen, k)
            assert np.array_equal(_bits(v), _bits(dist_all[:, :k])), (method, pen, k)
        if method == "confidence" and nq >= 3:
            assert np.all(np.isnan(dist_all[2])) and np.array_equal(idx_all[2], np.arange(n))
    # the repeated row ties exactly across runs: its copies come in index order
    idx_all, dist_all = _stable(n, nq, d, "euclidean", "none")
    pos = [int(np.nonzero(idx_all[0] == r)[0][0]) for r in sorted({1, min(16384, n - 1), n - 1})]
    assert pos == sorted(pos) and len(set(_bits(dist_all[0, pos]).tolist())) == 1


def test_ranking_of_seven_unequal_runs():
    n, nq, d = 100003, 2, 34
    idx_all, dist_all = _stable(n, nq, d, "euclidean", "none")
    for k in (n, 1025):
        i, v, _ = _rank_any(n, nq, d, "euclidean", "none", k)
        assert np.array_equal(i, idx_all[:, :k]) and np.array_equal(_bits(v), _bits(dist_all[:, :k]))


@pytest.mark.parametrize("n", (16385, 40000))
def test_first_1024_equal_pose_topk(n):
    db, q, _ = _data(n, 5, 34)
    ti, tv = torch.ops.stlpose.pose_topk(q, None, db, "euclidean", "none", 1024)
    i, v, _ = _rank_any(n, 5, 34, "euclidean", "none", 1024)
    assert np.array_equal(i, ti.cpu().numpy()) and np.array_equal(_bits(v), _bits(tv.cpu().numpy()))


def _labels(n, rows, seed=5):
    """int32 [2, n]: level 0 has 7 classes; level 1 has 3 and one more that only rows[0] carries (that query scores -1)."""
    rng = np.random.default_rng(seed)
    lab = np.stack([rng.integers(0, 7, n), rng.integers(0, 3, n)]).astype(np.int32)
    lab[1, rows[0]] = 99
    return lab


@pytest.mark.parametrize("n", (16384, 1000))
def test_equals_pose_rank_where_both_run(n):
    db, _, _ = _data(n, 5, 34)
    rows = [3, 0, n // 2, n - 1, 17]
    lab = _labels(n, rows)
    labels, qlabels = _cuda(lab, torch.int32), _cuda(lab[:, rows], torch.int32)
    q = db[rows]
    for k_eff in (n, 500):
        a = torch.ops.stlpose.pose_rank_any(q, None, db, "manhattan", "mean", n, labels, qlabels, k_eff)
        b = torch.ops.stlpose.pose_rank(q, None, db, "manhattan", "mean", n, labels, qlabels, k_eff)
        assert torch.equal(a[0], b[0])
        assert np.array_equal(_bits(a[1].cpu().numpy()), _bits(b[1].cpu().numpy()))
        assert np.array_equal(a[2].cpu().numpy().view(np.uint64), b[2].cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("n,atol", ((16385, 1e-11), (40000, 1e-11), (100003, 2e-11)))
def test_scores_equal_host_scoring_of_the_same_ranking(n, atol):
    """Count ratios are one fp64 division of the same integers on both sides: exactly equal.  mAP / mAR are means of at most n
    terms in [0, 1] summed in another order: within n * 2^-53 (1e-11 up to n = 40000, 2e-11 at 100003)."""
    from stlpose_amd.retrieval import _score_rows
    db, _, _ = _data(n, 2, 34)
    rows = [5, 0, 16384, n - 1, n // 2]
    lab = _labels(n, rows)
    labels, qlabels = _cuda(lab, torch.int32), _cuda(lab[:, rows], torch.int32)
    for k_eff in (n, 5000):
        idx, _, s = torch.ops.stlpose.pose_rank_any(db[rows], None, db, "euclidean", "zero_coord", n, labels, qlabels, k_eff)
        idx2, _, s2 = torch.ops.stlpose.pose_rank_any(db[rows], None, db, "euclidean", "zero_coord", 0, labels, qlabels, k_eff)
        idx, s = idx.cpu().numpy(), s.cpu().numpy()
        assert idx2.shape == (5, 0) and np.array_equal(s.view(np.uint64), s2.cpu().numpy().view(np.uint64))
        for li in range(2):
            want = _score_rows((lab[li][idx[:, 1:k_eff]] == lab[li][rows][:, None]).astype(np.int64))
            print(n, k_eff, li, "max |mAP, mAR diff|", np.abs(s[:, li][:, MEAN_COLS] - want[:, MEAN_COLS]).max())
            assert np.array_equal(s[:, li][:, COUNT_COLS], want[:, COUNT_COLS]), (k_eff, li)
            assert np.all(np.abs(s[:, li][:, MEAN_COLS] - want[:, MEAN_COLS]) <= atol), (k_eff, li)
        assert np.all(s[0, 1] == -1.0) and np.all(s[1:, 1] != -1.0) and np.all(s[:, 0] != -1.0)


def test_two_calls_are_bitwise_equal():
    n = 40000
    db, q, conf = _data(n, 5, 34)
    lab = _labels(n, [0])
    labels, qlabels = _cuda(lab, torch.int32), _cuda(lab[:, :5], torch.int32)
    runs = [torch.ops.stlpose.pose_rank_any(q, conf, db, "confidence", "max", n, labels, qlabels, n) for _ in range(2)]
    (i0, v0, s0), (i1, v1, s1) = [[t.cpu().numpy() for t in r] for r in runs]
    assert np.array_equal(i0, i1) and np.array_equal(_bits(v0), _bits(v1)) and np.array_equal(s0.view(np.uint64), s1.view(np.uint64))


def test_retrieval_experiment_scores_the_full_ranking_above_16384():
    from stlpose_amd import retrieval_experiment
    from stlpose_amd.pose_database import rank_any_batch
    from stlpose_amd.retrieval import score_retrievals
    rng = np.random.default_rng(11)
    n = 16385
    # values on a 1/8 grid: every squared distance is exact in fp32 and fp64, so both sides see the same order (ties by index)
    feats = (rng.integers(-8, 9, (n, 34)) / 8).astype(np.float32)
    chars = [f"c{v}" for v in rng.integers(0, 30, n)]
    chars[7] = "only_once"
    narr = [f"n{v}" for v in rng.integers(0, 5, n)]
    res = retrieval_experiment(feats, {"character": chars, "narrative": narr}, "all_kpts", "euclidean_distance", "zero_coord",
                               num_retrievals=-1, batch=4096)
    assert len(res["character"]) == n and len(res["narrative"]) == n
    f64 = feats.astype(np.float64)
    step = rank_any_batch(n, 4096)                 # the workspace budget may lower the batch: the samples sit on its boundaries
    assert 1 < step <= 4096 and n > 2 * step
    for qi in (0, 7, step - 1, step, 3 * step, n - 1):   # first and last query of a batch, and of the last, short batch
        order = np.argsort(np.sqrt(((f64[qi] - f64) ** 2).sum(1)), kind="stable")
        for level, labs in (("character", chars), ("narrative", narr)):
            want, got = score_retrievals(labs[qi], [labs[j] for j in order]), res[level][qi]
            assert got["label"] == labs[qi]
            for k in KEYS:
                if k in ("mAP", "mAR"):
                    assert abs(got[k] - want[k]) <= 1e-11, (level, qi, k)
                else:
                    assert got[k] == want[k], (level, qi, k)
    assert all(res["character"][7][k] == -1 for k in KEYS)


def test_first_k_search_above_1024_neighbours_and_16384_rows():
    from stlpose_amd import PoseIndex, get_neighbors_idxs
    from stlpose_amd.pose_database import search
    n, k = 20000, 2000
    db, q, _ = _data(n, 5, 34)
    idx_all, dist_all = _stable(n, 5, 34, "euclidean", "none")
    i, v = search(q, db, k, "euclidean", "none")
    assert np.array_equal(i.cpu().numpy(), idx_all[:, :k]) and np.array_equal(_bits(v.cpu().numpy()), _bits(dist_all[:, :k]))
    gi, gv = get_neighbors_idxs(q.cpu().numpy(), num_retrievals=k, approach="all_kpts", retrieval_method="euclidean_distance",
                                penalization="none", database=db.cpu().numpy())
    assert gi.shape == (5, k) and np.array_equal(gi, idx_all[:, :k]) and np.array_equal(_bits(gv), _bits(dist_all[:, :k]))
    g1, _ = get_neighbors_idxs(q[0].cpu().numpy(), num_retrievals=k, approach="all_kpts", retrieval_method="euclidean_distance",
                               penalization="none", database=db.cpu().numpy())
    assert np.array_equal(g1, idx_all[0, :k])
    index = PoseIndex(space="l2", dim=34)
    index.init_index(max_elements=n)
    index.add_items(db.cpu().numpy())
    li, ld = index.knn_query(q.cpu().numpy(), k=k)
    dd = torch.ops.stlpose.pose_distances(q, None, db, "l2sq", "zero_coord").cpu().numpy()
    order = np.argsort(dd, axis=1, kind="stable")[:, :k]
    assert np.array_equal(li.astype(np.int64), order) and np.array_equal(_bits(ld), _bits(np.take_along_axis(dd, order, 1)))
