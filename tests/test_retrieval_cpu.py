"""CPU: the retrieval fixture's generator, host scoring / aggregation, and argument validation that needs no GPU."""
import glob
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "retrieval", "g13_retrieval.npz")


@pytest.fixture(scope="module")
def built_lib():
    from stlpose_amd import build, capi
    build.build(verbose=False)
    return capi.lib()


KEYS = ("p@1", "p@5", "p@10", "p@rel", "mAP", "r@1", "r@5", "r@10", "r@rel", "mAR")


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference tree exists in the build container only")
def test_retrieval_generator_reproduces_fixture(tmp_path):
    env = dict(os.environ, STL_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "retrieval", "make_golden_retrieval.py")], check=True,
                   env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=600)
    a, b = np.load(FIX), np.load(os.path.join(str(tmp_path), "g13_retrieval.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    assert not glob.glob("/root/reference/**/__pycache__", recursive=True)


def test_fixture_layout():
    g = np.load(FIX)
    assert g["db"].shape == (300, 26) and g["q"].shape[1] == 26
    assert (g["joints_db"][:, :, :2] == 0).any() and (g["joints_q"][:, :, :2] == 0).any()
    assert len([k for k in g.files if k.startswith("idx_")]) == 5 * 4 * 2


def test_host_score_retrievals_matches_fixture():
    from stlpose_amd.retrieval import score_retrievals
    g = np.load(FIX)
    for row, want in zip(g["score_labels"], g["score_values"]):
        got = score_retrievals(int(row[0]), [int(x) for x in row])
        np.testing.assert_allclose([got[k] for k in KEYS], want, rtol=0, atol=1e-15)
    assert np.all(g["score_values"][6] == -1)


def test_host_score_retrievals_hand_cases():
    from stlpose_amd.retrieval import score_retrievals, _score_rows
    # query "a"; ranks 1.. = a b a b b b b b b b  -> relevant at positions 0 and 2
    s = score_retrievals("a", ["a", "a", "b", "a"] + ["b"] * 8)
    assert s["p@1"] == 1.0 and s["p@5"] == 2 / 5 and s["p@10"] == 2 / 10 and s["p@rel"] == 1 / 2
    assert s["mAP"] == pytest.approx((1 + 2 / 3) / 2) and s["r@1"] == 0.5 and s["r@5"] == 1.0 and s["mAR"] == pytest.approx(0.75)
    assert score_retrievals("z", ["z"] + ["y"] * 11)["mAP"] == -1
    rel = np.array([[1, 0, 1] + [0] * 9, [0] * 12])
    rows = _score_rows(rel)
    np.testing.assert_allclose(rows[0], [s[k] for k in KEYS], rtol=0, atol=1e-15)
    assert np.all(rows[1] == -1)


def test_process_retrieval_results_aggregates_like_reference(tmp_path):
    from stlpose_amd.retrieval import process_retrieval_results
    scores = [{"label": "a", **{k: 0.5 for k in KEYS}}, {"label": "a", **{k: 1.0 for k in KEYS}},
              {"label": "b", **{k: -1 for k in KEYS}}]
    params = types.SimpleNamespace(database_file="database_arch_data_eval.pkl", retrieval_method="euclidean_distance",
                                   approach="full_body", penalization="none", normalize=True)
    d = process_retrieval_results(scores, str(tmp_path), params, 1.5, 3, type="character")
    assert d["results"]["general"]["mAP"] == 0.75 and d["results"]["a"]["p@1"] == 0.75 and d["results"]["b"]["mAR"] == -1
    fname = "retrieval_results_type_character_method_euclidean_distance_approach_full_body_penalization_none_normalized_True.json"
    on_disk = json.load(open(os.path.join(str(tmp_path), fname)))
    assert on_disk["metadata"]["dataset_name"] == "arch_data" and on_disk["metadata"]["database size"] == 3
    assert set(on_disk["metadata"]) == {"timestamp", "dataset_name", "retrival_time", "database size", "retrieval_level",
                                        "retrieval_method", "pose approach", "missing kpt penalization", "normalized poses"}


def test_argument_validation_needs_no_device():
    from stlpose_amd import get_neighbors_idxs, process_pose_vector, retrieval_experiment
    from stlpose_amd import capi
    q, db = np.zeros(26, np.float32), np.zeros((20, 26), np.float32)
    with pytest.raises(ValueError, match="penalization"):
        get_neighbors_idxs(q, 5, retrieval_method="euclidean_distance", penalization=None, database=db)
    with pytest.raises(ValueError, match="retrieval_method"):
        get_neighbors_idxs(q, 5, retrieval_method="hamming", penalization="none", database=db)
    with pytest.raises(ValueError, match="approach"):
        get_neighbors_idxs(q, 5, approach="legs", retrieval_method="euclidean_distance", penalization="none", database=db)
    with pytest.raises(ValueError, match="approach"):
        process_pose_vector(np.zeros((17, 3)), "legs")
    labels = {"character": ["x"] * 20}
    with pytest.raises(ValueError, match="11"):
        retrieval_experiment(db, labels, num_retrievals=10)
    with pytest.raises(ValueError, match="method"):
        retrieval_experiment(db, labels, method="hamming")
    with pytest.raises(ValueError, match="penalization"):
        retrieval_experiment(db, labels, penalization=None)
    assert capi.POSE_TOPK_MAX == 1024 and capi.POSE_RANK_MAX == 16384


def test_c_abi_refuses_bad_arguments(built_lib):
    """Argument checks of the C ABI run before any device work: null pointers are never touched."""
    import ctypes as C
    from stlpose_amd import capi
    L = capi.lib()
    assert L.stl_pose_topk_workspace(1, 100, 101, 26) < 0 and b"k =" in L.stl_last_error()
    assert L.stl_pose_topk_workspace(1, 5000, 1025, 26) < 0
    assert L.stl_pose_topk(None, None, None, 1, 100, 20, 0, 0, 5, None, None, None, 0, None) < 0
    assert b"D = 20" in L.stl_last_error()
    assert L.stl_pose_distances(None, None, None, None, 1, 10, 26, 9, 0, None) < 0 and b"method" in L.stl_last_error()
    assert L.stl_pose_distances(None, None, None, None, 1, 10, 26, 0, 7, None) < 0 and b"penalization" in L.stl_last_error()
    assert L.stl_pose_rank(None, None, None, 1, 16385, 26, 0, 0, 0, None, None, None, None, 0, 0, None, None) < 0
    assert b"16384" in L.stl_last_error()
    lab = (C.c_int32 * 20)()
    assert L.stl_pose_rank(None, None, None, 1, 20, 26, 0, 0, 0, None, None, lab, lab, 1, 10, lab, None) < 0
    assert b"k_eff" in L.stl_last_error()
    assert L.stl_pose_vectors(None, 51, 3, None, 4, 5, 1, None) < 0 and b"approach" in L.stl_last_error()


def test_shape_mismatches_raise_before_any_launch():
    """The C ABI reads db rows with the query's width D and conf / labels by (Q, N): every mismatch is refused in the op wrappers
    (run here on host tensors: the checks come before any pointer reaches the library)."""
    import torch
    from stlpose_amd import PoseIndex, ops, retrieval_experiment
    q34, q26, db26 = torch.zeros(3, 34), torch.zeros(3, 26), torch.zeros(50, 26)
    with pytest.raises(RuntimeError, match="width"):
        ops._pose_topk(q34, None, db26, "euclidean", "none", 5)
    with pytest.raises(RuntimeError, match="width"):
        ops._pose_distances(q34, None, db26, "euclidean", "none")
    with pytest.raises(RuntimeError, match="width"):
        ops._pose_rank(q34, None, db26, "euclidean", "none", 5, None, None, 0)
    with pytest.raises(RuntimeError, match="2-D"):
        ops._pose_topk(torch.zeros(26), None, db26, "euclidean", "none", 5)
    with pytest.raises(RuntimeError, match="confidence"):
        ops._pose_topk(q26, torch.ones(3, 34), db26, "confidence", "none", 5)
    lab = torch.zeros(2, 50, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="labels"):
        ops._pose_rank(q26, None, db26, "euclidean", "none", 0, torch.zeros(2, 49, dtype=torch.int32), lab[:, :3], 20)
    with pytest.raises(RuntimeError, match="qlabels"):
        ops._pose_rank(q26, None, db26, "euclidean", "none", 0, lab, lab[:1, :3], 20)
    with pytest.raises(RuntimeError, match="qlabels"):
        ops._pose_rank(q26, None, db26, "euclidean", "none", 0, lab, None, 20)
    with pytest.raises(RuntimeError, match="joints"):
        ops._pose_vectors(torch.zeros(4, 16, 3), "full_body", True)
    with pytest.raises(RuntimeError, match="dimensionality"):
        PoseIndex(space="l2", dim=26).knn_query(np.zeros((2, 34), np.float32), k=1)
    with pytest.raises(ValueError, match="confidence"):
        retrieval_experiment(np.zeros((20, 26), np.float32), {"c": ["x"] * 20}, method="confidence_score",
                             confidence=np.ones((20, 34), np.float32))
