#!/usr/bin/env python3
"""Generate g13_retrieval.npz by running the REFERENCE's own lib/pose_database.py and lib/metrics.py.

Runs only where the reference tree exists.  Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/retrieval/make_golden_retrieval.py
(STL_GOLDEN_OUT=<dir> writes elsewhere).  hnswlib, pycocotools*, torchvision*, cv2 and data.* are replaced by empty stub modules
(the retrieval functions do not use them); CONFIG and lib.logger are the reference's own.  Only inputs and outputs are stored.

Contents (continuous random data, so no exact distance ties meet the reference's unstable np.argsort):
  joints_db [N,17,3] / joints_q [NQ,17,3] float32 with occluded (exactly 0) keypoints; vec_<approach>_<norm> [N, D];
  db / q: full_body normalised vectors; conf [NQ, D]; for every metric x penalization at num_retrievals 12 and N:
  idx_<m>_<p>_<k> [NQ, k], dist_<m>_<p>_<k> [NQ, k] (float64); score_* for score_retrievals cases.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("STL_GOLDEN_OUT") or HERE
REF = "/root/reference/src"
sys.dont_write_bytecode = True

N, NQ = 300, 6
METRICS = ("euclidean_distance", "cosine_similarity", "manhattan_distance", "confidence_score", "oks_score")
PENS = ("zero_coord", "none", "mean", "max")
SCORE_KEYS = ("p@1", "p@5", "p@10", "p@rel", "mAP", "r@1", "r@5", "r@10", "r@rel", "mAR")


def _import_reference():
    for name in ("hnswlib", "pycocotools", "pycocotools.coco", "pycocotools.cocoeval", "torchvision", "torchvision.transforms",
                 "cv2", "data", "data.data_processing"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pycocotools.coco"].COCO = object
    sys.modules["pycocotools.cocoeval"].COCOeval = object
    sys.path.insert(0, REF)
    import lib.metrics as metrics
    import lib.pose_database as pdb
    return pdb, metrics


def joints(rng, n):
    j = np.zeros((n, 17, 3), np.float32)
    j[:, :, :2] = rng.uniform(0.0, 1.0, (n, 17, 2)).astype(np.float32)
    j[:, :, 2] = 1.0
    occ = rng.uniform(size=(n, 17)) < 0.15
    occ[:, 5] &= rng.uniform(size=n) < 0.3   # the full_body / upper_body origin is occluded less often
    j[occ, :2] = 0.0
    return j


def main():
    pdb, metrics = _import_reference()
    rng = np.random.default_rng(20261015)
    jd, jq = joints(rng, N), joints(rng, NQ)
    out = {"joints_db": jd, "joints_q": jq}
    for ap in ("all_kpts", "full_body", "upper_body"):
        for norm in (True, False):
            out[f"vec_{ap}_{int(norm)}"] = np.stack([pdb.process_pose_vector(np.copy(j), ap, norm) for j in jd])
    db = out["vec_full_body_1"]
    q = np.stack([pdb.process_pose_vector(np.copy(j), "full_body", True) for j in jq])
    conf = rng.uniform(0.2, 1.0, q.shape).astype(np.float32)
    out["db"], out["q"], out["conf"] = db, q, conf
    for m in METRICS:
        for p in PENS:
            for k in (12, N):
                ii, dd = [], []
                for i in range(NQ):
                    kw = {"scores": conf[i]} if m == "confidence_score" else {}
                    idx, dist = pdb.get_neighbors_idxs(q[i], num_retrievals=k, approach="full_body", retrieval_method=m,
                                                       penalization=p, database=db, **kw)
                    ii.append(np.asarray(idx, np.int64)), dd.append(np.asarray(dist, np.float64))
                out[f"idx_{m}_{p}_{k}"], out[f"dist_{m}_{p}_{k}"] = np.stack(ii), np.stack(dd)
    # score_retrievals: random label lists, one query whose label never reappears, one all-relevant list
    labs = rng.integers(0, 5, (8, 40))
    labs[6, 1:] = np.where(labs[6, 1:] == labs[6, 0], (labs[6, 0] + 1) % 5, labs[6, 1:])
    labs[7] = labs[7, 0]
    out["score_labels"] = labs
    out["score_values"] = np.array([[metrics.score_retrievals(int(r[0]), [int(x) for x in r])[k] for k in SCORE_KEYS] for r in labs],
                                   np.float64)
    np.savez(os.path.join(OUT, "g13_retrieval.npz"), **out)


if __name__ == "__main__":
    main()
