"""Host (numpy, float64) restatement of the reference's retrieval semantics for the retrieval tests: pose vectors,
the five metrics with their penalizations (lib/pose_database.py:149-285, lib/metrics.py:97-149) and the all-vs-all
experiment with a STABLE argsort (the reference's np.argsort is unstable; the GPU's order is the stable one)."""
from __future__ import annotations

import numpy as np

KPTS = {"all_kpts": list(range(17)), "full_body": list(range(5, 17)) + [0], "upper_body": list(range(5, 13)) + [0]}
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
EPS = 1e-5


def pose_vectors(joints, approach, normalize):
    v = np.asarray(joints, np.float64)[:, KPTS[approach], :2].reshape(len(joints), -1)
    zero = v == 0
    v = v - np.tile(v[:, :2], v.shape[1] // 2)
    v[zero] = 0
    if normalize:
        v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), EPS)
    return v


def metric(method, q, x, c):
    d = len(q)
    if method == "euclidean":
        return np.sqrt(np.sum((q - x) ** 2))
    if method == "cosine":
        return 1 - np.dot(q, x)
    if method == "manhattan":
        return np.sum(np.abs(q - x))
    if method == "confidence":
        c = c / np.sqrt(np.sum(c ** 2))
        return np.sqrt(np.sum(c * (q - x) ** 2)) / np.sum(c)
    if method == "oks":
        kp = KPTS["all_kpts" if d == 34 else "full_body" if d == 26 else "upper_body"]
        sq = (q[0::2] - x[0::2]) ** 2 + (q[1::2] - x[1::2]) ** 2
        return 1 - np.sum(np.exp(-sq / (SIGMAS[kp] ** 2 * 2))) / (d // 2)
    if method == "l2sq":
        return np.sum((q - x) ** 2)
    if method == "cos_normalised":
        return 1 - np.dot(q, x) / ((np.linalg.norm(q) + 1e-30) * (np.linalg.norm(x) + 1e-30))
    raise ValueError(method)


def distances(method, pen, q, db, c=None):
    """[N] distances of one query, fp64."""
    q, db = np.asarray(q, np.float64), np.asarray(db, np.float64)
    c = np.ones_like(q) if c is None or method == "oks" else np.asarray(c, np.float64)
    pv = 0.0
    if pen in ("mean", "max") and method not in ("l2sq", "cos_normalised"):
        vals = [metric(method, q, x, c) for x in db[:100]]
        pv = np.mean(vals) if pen == "mean" else np.max(vals)
    out = np.empty(len(db))
    for i, x in enumerate(db):
        qq, xx, cc = q.copy(), x.copy(), c.copy()
        if method not in ("l2sq", "cos_normalised"):
            if pen == "none":
                m = np.abs(q) < EPS
                qq[m], xx[m], cc[m] = 0, 0, 0
            elif pen in ("mean", "max"):
                m = (np.abs(q) < EPS) & (np.abs(x) > EPS)
                qq[m], xx[m], cc[m] = pv, 0, 0
        out[i] = metric(method, qq, xx, cc)
    return out


def score(label, ranked_labels):
    rel = (np.asarray(ranked_labels)[1:] == label).astype(np.int64)
    nrel = rel.sum()
    if nrel == 0:
        return [-1.0] * 10
    hits = np.cumsum(rel)
    p, r = hits / np.arange(1, len(rel) + 1), hits / nrel
    return [p[0], p[4], p[9], p[nrel - 1], np.sum(p * rel) / nrel, r[0], r[4], r[9], r[nrel - 1], np.sum(r * rel) / nrel]
