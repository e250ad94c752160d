"""Pose-based retrieval experiment on the GPU: drop-in for ``src/07_retrieval_experiments.py`` (RetrievalExp) and
``lib/metrics.py:score_retrievals``.

``retrieval_experiment`` ranks every pose against the whole database and scores the rankings per label level inside the
``stlpose::pose_rank`` kernel (N <= 16384): no [N, N] array is ever written.  Above that size it runs ``stlpose::pose_topk``
and scores the returned rankings on the host when num_retrievals <= 1024, and ``stlpose::pose_rank_any`` otherwise (the full
ranking included): sorted runs merged in a global workspace, scores on the device, queries batched so that the workspace stays
under ``pose_database.RANK_WORKSPACE_BUDGET`` (1 GiB).
"""
from __future__ import annotations

import copy
import json
import os
import time
from typing import Dict, Sequence

import numpy as np
import torch

from . import capi
from . import ops  # noqa: F401
from .pose_database import METHODS, PENALIZATIONS, _check_approach, _dev, rank_any_batch

SCORE_KEYS = ("p@1", "p@5", "p@10", "p@rel", "mAP", "r@1", "r@5", "r@10", "r@rel", "mAR")   # STL_POSE_NSCORES, kernel order


def score_retrievals(label, retrievals) -> dict:
    """metrics.py:25-94 on the host: precision / recall metrics of one ranked list of labels, rank 0 (self-retrieval) dropped.
    A query with no relevant retrieval scores -1 everywhere."""
    rel = np.array([1 if r == label else 0 for r in list(retrievals)[1:]])
    nrel = int(rel.sum())
    if nrel == 0:
        return {"label": label, **{k: -1 for k in SCORE_KEYS}}
    hits = np.cumsum(rel)
    prec = hits / np.arange(1, len(rel) + 1)
    rec = hits / nrel
    vals = (prec[0], prec[4], prec[9], prec[nrel - 1], np.sum(prec * rel) / nrel,
            rec[0], rec[4], rec[9], rec[nrel - 1], np.sum(rec * rel) / nrel)
    return {"label": label, **dict(zip(SCORE_KEYS, vals))}


def _score_rows(rel: np.ndarray) -> np.ndarray:
    """score_retrievals for a batch of relevance rows [Q, m] (rank 0 already dropped) -> [Q, 10] fp64."""
    hits = np.cumsum(rel, axis=1)
    nrel = hits[:, -1]
    safe = np.maximum(nrel, 1)[:, None].astype(np.float64)
    prec = hits / np.arange(1, rel.shape[1] + 1)
    rec = hits / safe
    at = np.take_along_axis(hits, np.maximum(nrel - 1, 0)[:, None], axis=1)[:, 0]
    out = np.stack([prec[:, 0], prec[:, 4], prec[:, 9], at / safe[:, 0], (prec * rel).sum(1) / safe[:, 0],
                    rec[:, 0], rec[:, 4], rec[:, 9], at / safe[:, 0], (rec * rel).sum(1) / safe[:, 0]], axis=1)
    out[nrel == 0] = -1.0
    return out


def _label_ids(labels) -> tuple:
    """{level: labels[N]} or [labels[N], ...] -> (level names, int32 [L, N] ids, per level the id -> label table)."""
    items = list(labels.items()) if isinstance(labels, dict) else [(f"level{i}", v) for i, v in enumerate(labels)]
    names, ids, tables = [], [], []
    for name, vals in items:
        uniq, inv = np.unique(np.asarray(list(vals)), return_inverse=True)
        names.append(name), ids.append(inv.astype(np.int32)), tables.append(uniq)
    return names, np.stack(ids), tables


def retrieval_experiment(features, labels, approach: str = "full_body", method: str = "euclidean_distance",
                         penalization: str = "zero_coord", num_retrievals: int = -1, batch: int = 2048,
                         confidence=None) -> Dict[str, list]:
    """RetrievalExp.retrieval_experiment (07_retrieval_experiments.py:67-112), batched on the GPU.

    features: [N, D] pose vectors (every pose is a query against all of them); labels: {level: per-pose labels} (e.g.
    {"character": ..., "narrative": ...}) or a list of such sequences, at most 4 levels.  method: the reference's retrieval_method
    names (or the kernel's own); num_retrievals = -1 scores the full ranking; batch: queries per launch (fewer where the
    workspace of a ranking above N = 16384 would pass its budget).  Returns {level: [score_retrievals dict per query]}
    in query order, and the elapsed seconds under the key "elapsed_time"."""
    _check_approach(approach)
    m = METHODS.get(method, method)
    if m not in capi.POSE_METHOD:
        raise ValueError(f"method {method!r}: expected one of {tuple(METHODS)}")
    if penalization not in PENALIZATIONS:
        raise ValueError(f"penalization {penalization!r}: expected one of {PENALIZATIONS}")
    if len(features.shape) != 2:
        raise ValueError(f"features must be [N, D], got {tuple(features.shape)}")
    if confidence is not None and tuple(np.shape(confidence)) != tuple(features.shape):
        raise ValueError(f"confidence must have the features' shape {tuple(features.shape)}, got {tuple(np.shape(confidence))}")
    names, ids, tables = _label_ids(labels)
    n = int(features.shape[0])
    if ids.shape[1] != n:
        raise ValueError(f"{ids.shape[1]} labels for {n} poses")
    if len(names) > capi.POSE_RANK_LABELS_MAX:
        raise ValueError(f"at most {capi.POSE_RANK_LABELS_MAX} label levels")
    k_eff = n if num_retrievals < 0 else int(num_retrievals)
    if k_eff < 11 or k_eff > n:
        raise ValueError(f"num_retrievals = {num_retrievals}: scoring needs 11 <= retrievals <= N = {n} (p@10 reads rank 10)")
    rank_any = n > capi.POSE_RANK_MAX and k_eff > capi.POSE_TOPK_MAX
    if rank_any:
        if n > capi.POSE_RANK_ANY_MAX:
            raise ValueError(f"N = {n} > {capi.POSE_RANK_ANY_MAX}: a ranking longer than {capi.POSE_TOPK_MAX} is not supported")
        batch = rank_any_batch(n, batch)
    start = time.time()
    db = _dev(features)
    conf = _dev(confidence) if confidence is not None else None
    lab = _dev(ids, torch.int32)
    scores = np.empty((n, len(names), capi.POSE_NSCORES))
    for q0 in range(0, n, batch):
        q1 = min(n, q0 + batch)
        c = conf[q0:q1] if conf is not None else None
        if n <= capi.POSE_RANK_MAX:
            _, _, s = torch.ops.stlpose.pose_rank(db[q0:q1], c, db, m, penalization, 0, lab, lab[:, q0:q1], k_eff)
            scores[q0:q1] = s.cpu().numpy()
        elif rank_any:
            _, _, s = torch.ops.stlpose.pose_rank_any(db[q0:q1], c, db, m, penalization, 0, lab, lab[:, q0:q1], k_eff)
            scores[q0:q1] = s.cpu().numpy()
        else:
            idx, _ = torch.ops.stlpose.pose_topk(db[q0:q1], c, db, m, penalization, k_eff)
            idx = idx.cpu().numpy()
            for li in range(len(names)):
                rel = (ids[li][idx[:, 1:]] == ids[li][q0:q1, None]).astype(np.int64)
                scores[q0:q1, li] = _score_rows(rel)
    elapsed = time.time() - start
    out: Dict[str, list] = {"elapsed_time": elapsed}
    for li, name in enumerate(names):
        out[name] = [{"label": tables[li][ids[li][i]].item(), **{k: _num(scores[i, li, j]) for j, k in enumerate(SCORE_KEYS)}}
                     for i in range(n)]
    return out


def _num(v: float):
    return -1 if v == -1.0 else float(v)


def process_retrieval_results(scores: Sequence[dict], exp_directory: str, params, elapsed_time: float, n_entries: int,
                              type: str = "character", save: bool = True) -> dict:
    """RetrievalExp.process_retrieval_results (07_retrieval_experiments.py:114-175): per-label means and a "general" mean that
    skips the -1 entries; written to the reference's JSON file name and keys.  params: has database_file, retrieval_method,
    approach, penalization, normalize."""
    if type not in ("character", "narrative"):
        raise ValueError("type must be 'character' or 'narrative'")
    template = {k: [] for k in SCORE_KEYS}
    results = {"general": copy.deepcopy(template)}
    for s in scores:
        lab = s["label"]
        if lab not in results:
            results[lab] = copy.deepcopy(template)
        for k in SCORE_KEYS:
            results[lab][k].append(s[k])
            if s[k] >= 0:
                results["general"][k].append(s[k])
    with np.errstate(all="ignore"):
        for r in results.values():
            for k in SCORE_KEYS:
                r[k] = float(np.mean(r[k])) if len(r[k]) else float("nan")
    dataset_name = params.database_file.split("database_")[1].split("_eval")[0]
    savedict = {
        "results": results,
        "metadata": {
            "timestamp": time.strftime("%Y-%m-%d_%H-%M-%S"),
            "dataset_name": dataset_name,
            "retrival_time": elapsed_time,
            "database size": n_entries,
            "retrieval_level": type,
            "retrieval_method": params.retrieval_method,
            "pose approach": params.approach,
            "missing kpt penalization": params.penalization,
            "normalized poses": params.normalize,
        },
    }
    if save:
        fname = (f"retrieval_results_type_{type}_method_{params.retrieval_method}_approach_{params.approach}_"
                 f"penalization_{params.penalization}_normalized_{params.normalize}.json")
        with open(os.path.join(exp_directory, fname), "w") as f:
            json.dump(savedict, f)
    return savedict
