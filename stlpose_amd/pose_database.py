"""Pose database and exact k-NN search on the GPU: drop-in for the reference's ``lib/pose_database.py`` and its use of hnswlib
(``src/06_fit_knn_tree.py``).

Every distance, selection and sort runs in the HIP kernels of ``csrc/retrieval.hip`` (ops ``stlpose::pose_vectors``,
``pose_distances``, ``pose_topk``, ``pose_rank``, ``pose_rank_any``).  The search is EXACT: the neighbours are the first k of a
stable argsort of all distances (ties by ascending database index, NaN last), where the reference's hnswlib graph is approximate.
Any k <= N is served at any N <= 2^24: k <= 1024 by the fused top-k kernel, larger k by a full ranking, in one workgroup's LDS up
to N = 16384 and through sorted runs merged in a global workspace above (queries batched to keep it under
``RANK_WORKSPACE_BUDGET``).

:class:`PoseIndex` stands in for the subset of ``hnswlib.Index`` the reference uses.  Its file format (``save_index``) is our own: an
uncompressed numpy ``.npz`` written to exactly the given path, with the arrays

    format        str   "stlpose_pose_index"
    version       int64 1
    space         str   "l2" | "cosine"
    dim           int64 vector dimension
    max_elements  int64 capacity given to init_index
    data          float32 [count, dim] the vectors as added
    ids           uint64 [count] their labels
"""
from __future__ import annotations

import os
import pickle
from typing import Optional, Tuple

import numpy as np
import torch

from . import capi
from . import ops  # noqa: F401  (registers the stlpose:: ops)

# reference retrieval_method names -> kernel metric (include/stlpose_hip.h STL_POSE_*)
METHODS = {"euclidean_distance": "euclidean", "cosine_similarity": "cosine", "manhattan_distance": "manhattan",
           "confidence_score": "confidence", "oks_score": "oks"}
PENALIZATIONS = ("zero_coord", "none", "mean", "max")
APPROACHES = tuple(capi.POSE_APPROACH)
SPACES = {"l2": "l2sq", "cosine": "cos_normalised"}
RANK_WORKSPACE_BUDGET = 1 << 30   # bytes of pose_rank_any workspace (16 B per query and database row) one launch may take


def rank_any_batch(n: int, batch: int, budget: int = None) -> int:
    """Queries per ``pose_rank_any`` call at database size n: at most `batch`, the C ABI's 65535, and what fits the budget."""
    per_query = capi.lib().stl_pose_rank_any_workspace(1, n)
    capi.check(min(per_query, 0), "stl_pose_rank_any")
    budget = RANK_WORKSPACE_BUDGET if budget is None else budget
    return max(1, min(int(batch), 65535, budget // per_query))


def _check_approach(approach: str) -> None:
    if approach not in capi.POSE_APPROACH:
        raise ValueError(f"approach {approach!r}: expected one of {APPROACHES}")


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def _dev(x, dtype=torch.float32) -> torch.Tensor:
    """numpy / list / tensor -> contiguous tensor on the current GPU."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=_device(), dtype=dtype).contiguous()


def process_pose_vectors(joints, approach: str = "full_body", normalize: bool = True) -> torch.Tensor:
    """Batched pose vectors (06_fit_knn_tree.py:84-147): joints [N, 17, C >= 2] (tensor or numpy) -> float32 [N, D] on the GPU."""
    _check_approach(approach)
    j = _dev(joints)
    if j.dim() != 3 or j.shape[1] != 17 or j.shape[2] < 2:
        raise ValueError(f"joints must be [N, 17, C >= 2], got {tuple(j.shape)}")
    return torch.ops.stlpose.pose_vectors(j, approach, bool(normalize))


def process_pose_vector(vector, approach: str, normalize: bool = True) -> np.ndarray:
    """One pose (pose_database.py:19-69): numpy [17, C >= 2] in, numpy float32 [D] out."""
    v = np.asarray(vector)
    if v.ndim != 2:
        raise ValueError(f"process_pose_vector takes one [17, C] joints array, got shape {v.shape}")
    return process_pose_vectors(v[None], approach, normalize)[0].cpu().numpy()


def _num_out(num_retrievals: int, n: int) -> int:
    """How many entries the reference's ``np.argsort(dists)[:num_retrievals]`` keeps (Python slice semantics, -1 included)."""
    return len(range(n)[:num_retrievals])


def search(query, database, k: int, method: str = "euclidean", penalization: str = "zero_coord", confidence=None
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact first-k search on the GPU: (idx int64 [Q, k], dist float32 [Q, k]).  k <= 1024 runs the fused top-k kernel at any
    N; larger k a full ranking: ``pose_rank`` up to N = 16384, ``pose_rank_any`` above, in query batches of
    ``rank_any_batch(N, 2048)``."""
    q, db = _dev(query), _dev(database)
    c = _dev(confidence) if confidence is not None else None
    n = db.shape[0]
    if k == 0:
        return (torch.empty(q.shape[0], 0, dtype=torch.int64, device=q.device),
                torch.empty(q.shape[0], 0, dtype=torch.float32, device=q.device))
    if k <= capi.POSE_TOPK_MAX:
        return torch.ops.stlpose.pose_topk(q, c, db, method, penalization, k)
    if n <= capi.POSE_RANK_MAX:
        idx, dist, _ = torch.ops.stlpose.pose_rank(q, c, db, method, penalization, k, None, None, 0)
        return idx, dist
    if n > capi.POSE_RANK_ANY_MAX:
        raise ValueError(f"a ranking of {k} > {capi.POSE_TOPK_MAX} entries needs N <= {capi.POSE_RANK_ANY_MAX} (N = {n})")
    step = rank_any_batch(n, 2048)
    parts = [torch.ops.stlpose.pose_rank_any(q[q0:q0 + step], c[q0:q0 + step] if c is not None else None, db, method, penalization, k,
                                             None, None, 0)[:2] for q0 in range(0, q.shape[0], step)]
    if not parts:
        return (torch.empty(0, k, dtype=torch.int64, device=q.device), torch.empty(0, k, dtype=torch.float32, device=q.device))
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def get_neighbors_idxs(query, num_retrievals: int = 10, approach: str = "full_body", retrieval_method: str = "knn",
                       penalization: Optional[str] = None, **kwargs):
    """Drop-in for pose_database.py:149-248 (same names, kwargs ``database``, ``knn``, ``scores``; returns (idx, dists)).

    query: one pose vector [D], or a batch [Q, D] (then idx / dists are [Q, k]).  Exact, on the GPU."""
    q = np.asarray(query, dtype=np.float32)
    single = q.ndim == 1
    q2 = q[None] if single else q
    if retrieval_method == "knn":
        if "knn" not in kwargs:
            raise ValueError("retrieval_method='knn' needs the index as knn=...")
        idx, dists = kwargs["knn"].knn_query(q2, k=num_retrievals)
        return (idx[0], dists[0]) if single else (idx, dists)
    if retrieval_method not in METHODS:
        raise ValueError(f"retrieval_method {retrieval_method!r}: expected 'knn' or one of {tuple(METHODS)}")
    if penalization not in PENALIZATIONS:
        raise ValueError(f"penalization {penalization!r}: expected one of {PENALIZATIONS} with retrieval_method={retrieval_method!r}")
    _check_approach(approach)
    if "database" not in kwargs:
        raise ValueError("'database' (the [N, D] pose vectors) was not given")
    database = kwargs["database"]
    method = METHODS[retrieval_method]
    conf = None
    if method == "confidence" and "scores" in kwargs:
        conf = np.broadcast_to(np.asarray(kwargs["scores"], dtype=np.float32), q2.shape)
    k = _num_out(num_retrievals, int(database.shape[0]))
    idx, dist = search(q2, database, k, method, penalization, conf)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    return (idx[0], dist[0]) if single else (idx, dist)


def get_penalization_metric(query, database, metric_func, penalization: str = "mean", confidence=None, N: int = 100):
    """pose_database.py:251-285 on the host: mean or max of ``metric_func(query, row, confidence)`` over the first N rows.  (The
    GPU kernels compute the same value per query inside their launch.)"""
    if penalization not in ("mean", "max"):
        raise ValueError(f"penalization {penalization!r}: expected 'mean' or 'max'")
    vals = [metric_func(query, row, confidence) for row in np.asarray(database)[:N]]
    return np.mean(vals) if penalization == "mean" else np.max(vals)


class PoseIndex:
    """Exact GPU stand-in for the ``hnswlib.Index`` calls of the reference (06_fit_knn_tree.py:150-166,
    pose_database.py:140-146,182-185).  space "l2" returns SQUARED L2 distances, "cosine" 1 - cos, as hnswlib does."""

    def __init__(self, space: str, dim: int):
        if space not in SPACES:
            raise ValueError(f"space {space!r}: expected 'l2' or 'cosine'")
        self.space, self.dim = space, int(dim)
        self.max_elements = 0
        self.ef = 10
        self._data = None   # float32 [count, dim] on the GPU
        self._ids = np.zeros(0, dtype=np.uint64)
        self._initialised = False

    def init_index(self, max_elements: int, ef_construction: int = 200, M: int = 16, random_seed: int = 100) -> None:
        """Graph tuning arguments are accepted and ignored: the search is exhaustive."""
        self.max_elements = int(max_elements)
        self._data = torch.empty(0, self.dim, dtype=torch.float32, device=_device())
        self._ids = np.zeros(0, dtype=np.uint64)
        self._initialised = True

    def set_ef(self, ef: int) -> None:
        self.ef = int(ef)

    def get_current_count(self) -> int:
        return 0 if self._data is None else int(self._data.shape[0])

    def get_max_elements(self) -> int:
        return self.max_elements

    def add_items(self, data, ids=None) -> None:
        if not self._initialised:
            raise RuntimeError("add_items before init_index")
        x = np.asarray(data, dtype=np.float32)
        x = x[None] if x.ndim == 1 else x
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise RuntimeError(f"wrong dimensionality of the vectors: {x.shape}, index dim {self.dim}")
        n0 = self.get_current_count()
        if n0 + x.shape[0] > self.max_elements:
            raise RuntimeError(f"the number of elements exceeds the specified limit ({self.max_elements})")
        new_ids = np.arange(n0, n0 + x.shape[0], dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64).reshape(-1)
        if new_ids.shape[0] != x.shape[0]:
            raise RuntimeError("ids and data differ in length")
        self._data = torch.cat([self._data, _dev(x)]) if n0 else _dev(x)
        self._ids = np.concatenate([self._ids, new_ids])

    def knn_query(self, data, k: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """(labels uint64 [Q, k], distances float32 [Q, k]), nearest first."""
        q = np.asarray(data, dtype=np.float32)
        q = q[None] if q.ndim == 1 else q
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise RuntimeError(f"wrong dimensionality of the query vectors: {q.shape}, index dim {self.dim}")
        count = self.get_current_count()
        if k < 1 or k > count:
            raise RuntimeError(f"cannot return {k} neighbours from an index of {count} elements")
        idx, dist = search(q, self._data, int(k), SPACES[self.space], "zero_coord")
        return self._ids[idx.cpu().numpy()], dist.cpu().numpy()

    def save_index(self, path: str) -> None:
        data = self._data.cpu().numpy() if self._data is not None else np.zeros((0, self.dim), np.float32)
        with open(path, "wb") as f:   # a file object: np.savez would append ".npz" to a bare path
            np.savez(f, format=np.array("stlpose_pose_index"), version=np.int64(1), space=np.array(self.space),
                     dim=np.int64(self.dim), max_elements=np.int64(self.max_elements), data=data, ids=self._ids)

    def load_index(self, path: str, max_elements: int = 0) -> None:
        """Load a file written by save_index.  The space stays the one this object was constructed with (hnswlib's rule);
        max_elements = 0 keeps the saved capacity."""
        z = np.load(path)
        if str(z["format"]) != "stlpose_pose_index" or int(z["version"]) != 1:
            raise RuntimeError(f"{path}: not a PoseIndex file")
        if int(z["dim"]) != self.dim:
            raise RuntimeError(f"{path}: dim {int(z['dim'])}, index dim {self.dim}")
        self.max_elements = max(int(max_elements), int(z["max_elements"]), int(z["data"].shape[0]))
        self._data = _dev(z["data"]).reshape(-1, self.dim)
        self._ids = z["ids"].astype(np.uint64)
        self._initialised = True


def _knn_names(database_file: str, metric: str, approach: str, normalize) -> str:
    tag = "" if approach == "full_body" else f"approach_{approach}_"
    return f"{os.path.basename(database_file)[:-4]}_metric_{metric}_norm_{tag}{normalize}.pkl"


def fit_knn_structure(processed_features, data, params, knn_dir: str) -> str:
    """06_fit_knn_tree.py:150-207: fit a PoseIndex on the features and write graph_<name>, data_<name> and features_<name> into
    knn_dir.  params: has database_file, metric ("euclidean_distance" | "cosine_similarity"), approach, normalize.  Returns <name>."""
    space = {"euclidean_distance": "l2", "cosine_similarity": "cosine"}.get(params.metric)
    if space is None:
        raise ValueError(f"metric {params.metric!r}: the index supports 'euclidean_distance' and 'cosine_similarity'")
    feats = np.asarray(processed_features.cpu() if isinstance(processed_features, torch.Tensor) else processed_features, np.float32)
    n, dim = feats.shape
    knn = PoseIndex(space=space, dim=dim)
    knn.init_index(max_elements=n, ef_construction=1000, M=8)
    knn.set_ef(1000)
    knn.add_items(feats, np.arange(n))
    name = _knn_names(params.database_file, params.metric, params.approach, params.normalize)
    knn.save_index(os.path.join(knn_dir, f"graph_{name}"))
    with open(os.path.join(knn_dir, f"data_{name}"), "wb") as f:
        pickle.dump(data, f)
    with open(os.path.join(knn_dir, f"features_{name}"), "wb") as f:
        pickle.dump(feats, f)
    return name


def load_knn(database_file: str, knn_dir: str):
    """pose_database.py:95-146: (knn, database, features) from the files fit_knn_structure wrote.  database_file is the
    'data_<name>' file name; the index is opened in space 'l2', as the reference does."""
    name = database_file[5:]
    paths = {k: os.path.join(knn_dir, f"{k}_{name}") for k in ("graph", "data", "features")}
    for k, p in paths.items():
        if not os.path.exists(p):
            raise FileNotFoundError(f"kNN {k} file '{p}' does not exist")
    with open(paths["data"], "rb") as f:
        database = pickle.load(f)
    with open(paths["features"], "rb") as f:
        features = pickle.load(f)
    knn = PoseIndex(space="l2", dim=features.shape[-1])
    knn.load_index(paths["graph"], max_elements=0)
    return knn, database, features
