#!/usr/bin/env python3
"""Pose retrieval benchmark (GPU only): `python tools/retrieval_bench.py OUTDIR` writes OUTDIR/retrieval_bench.json.

Cases (seeded uniform pose vectors, D = 26 = full_body):
  a  all-vs-all full ranking + scores (stlpose::pose_rank, 2 label levels), N = 8192, every method (penalization "none")
  b  fused top-k (stlpose::pose_topk), k = 10 and 100, Q = 8192 against N = 150000 (euclidean, zero_coord)
  c  one query against N = 150000, k = 10 and 100
  d  the same work composed from torch ops on the same GPU, euclidean: torch.cdist + topk (b, c) and cdist + sort(stable) (a)
  e  the reference-semantics numpy loop (per-query Python loop over the database, pose_database.py:220-248) on 20 queries,
     extrapolated linearly to the 8192 queries of (a)
Times are device events around `reps` launches after a warm-up.  Each case reports its cost model next to the numbers:
flops = 2 * D per pair (sub + fma); bytes = the HBM traffic the implementation cannot avoid -- the database, the queries and the
results once each (the database, N x 26 x 4 B <= 15.6 MB, stays in L2 / Infinity Cache across query tiles), plus, for the
torch-composed yardstick, writing and reading back its [Q, N] distance matrix.  "bound" names the larger of flops / peak and
bytes / peak, "share_of_peak" is that lower bound over the measured time; peaks from MI355X_MICROARCH.md: 157.3 TF fp32 vector,
8.0 TB/s HBM.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FLOPS, PEAK_BW = 157.3e12, 8.0e12
D = 26


def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def rates(sec, q, n, out_bytes, matrix=False):
    """q queries against n rows; out_bytes: results written; matrix: the [q, n] fp32 distances are written and read back."""
    pairs = q * n
    fl = 2.0 * D * pairs
    bytes_ = (q + n) * D * 4 + out_bytes + (2 * pairs * 4 if matrix else 0)
    t_f, t_b = fl / PEAK_FLOPS, bytes_ / PEAK_BW
    model = "database + queries + results once" + (" + [Q,N] distance matrix written and read" if matrix else "")
    return {"seconds": sec, "pairs_per_s": pairs / sec, "flops": fl, "bytes": bytes_, "bytes_model": model,
            "gflops": fl / sec / 1e9, "gbytes_per_s": bytes_ / sec / 1e9, "floor_compute_s": t_f, "floor_memory_s": t_b,
            "bound": "compute" if t_f >= t_b else "memory", "share_of_peak": max(t_f, t_b) / sec}


def main(outdir):
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench: no GPU")
    import stlpose_amd  # noqa: F401
    from stlpose_amd import capi
    import retrieval_ref as R
    os.makedirs(outdir, exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "D": D, "cases": {}}
    C = res["cases"]

    n = 8192
    db = torch.rand(n, D, device="cuda", generator=gen) * 2 - 1
    lab = torch.stack([torch.randint(0, 60, (n,), device="cuda", generator=gen),
                       torch.randint(0, 8, (n,), device="cuda", generator=gen)]).to(torch.int32)
    for m in ("euclidean", "cosine", "manhattan", "confidence", "oks"):
        conf = torch.rand(n, D, device="cuda", generator=gen) if m == "confidence" else None
        sec = timed(lambda: torch.ops.stlpose.pose_rank(db, conf, db, m, "none", 0, lab, lab, n), reps=2)
        C[f"a_rank_scores_{m}_N{n}"] = rates(sec, n, n, n * 2 * 10 * 8)
    sec = timed(lambda: torch.sort(torch.cdist(db, db), dim=1, stable=True), reps=2)
    C[f"d_torch_cdist_sort_stable_N{n}"] = rates(sec, n, n, n * n * 12, matrix=True)

    nb = 150000
    big = torch.rand(nb, D, device="cuda", generator=gen) * 2 - 1
    for k in (10, 100):
        q = big[:8192]
        sec = timed(lambda: torch.ops.stlpose.pose_topk(q, None, big, "euclidean", "zero_coord", k))
        C[f"b_topk_k{k}_Q8192_N{nb}"] = rates(sec, 8192, nb, 8192 * k * 12)
        sec = timed(lambda: torch.topk(torch.cdist(q, big), k, dim=1, largest=False, sorted=True))
        C[f"d_torch_cdist_topk_k{k}_Q8192_N{nb}"] = rates(sec, 8192, nb, 8192 * k * 12, matrix=True)
        q1 = big[:1]
        sec = timed(lambda: torch.ops.stlpose.pose_topk(q1, None, big, "euclidean", "zero_coord", k), reps=50, warm=5)
        C[f"c_topk_k{k}_Q1_N{nb}"] = rates(sec, 1, nb, k * 12)
        sec = timed(lambda: torch.topk(torch.cdist(q1, big), k, dim=1, largest=False, sorted=True), reps=50, warm=5)
        C[f"d_torch_cdist_topk_k{k}_Q1_N{nb}"] = rates(sec, 1, nb, k * 12, matrix=True)

    host = db[:2000].cpu().numpy().astype(np.float64)
    t0 = time.time()
    for i in range(20):
        d = R.distances("euclidean", "none", host[i], db.cpu().numpy())
        np.argsort(d)
    per_q = (time.time() - t0) / 20
    C[f"e_numpy_loop_euclidean_N{n}"] = {"seconds_per_query": per_q, "seconds_extrapolated_all_vs_all": per_q * n,
                                          "pairs_per_s": n / per_q}
    for k in (10, 100):
        C[f"b_vs_d_speedup_k{k}"] = C[f"d_torch_cdist_topk_k{k}_Q8192_N{nb}"]["seconds"] / C[f"b_topk_k{k}_Q8192_N{nb}"]["seconds"]
        C[f"c_vs_d_speedup_k{k}"] = C[f"d_torch_cdist_topk_k{k}_Q1_N{nb}"]["seconds"] / C[f"c_topk_k{k}_Q1_N{nb}"]["seconds"]
    res["topk_limits"] = {"k_max": capi.POSE_TOPK_MAX, "rank_n_max": capi.POSE_RANK_MAX}
    with open(os.path.join(outdir, "retrieval_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: retrieval_bench.py OUTDIR")
    main(sys.argv[1])
