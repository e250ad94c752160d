#!/usr/bin/env python3
"""Pose retrieval benchmark (GPU only): `python tools/retrieval_bench.py OUTDIR [all | classic | full_ranking]` writes
OUTDIR/retrieval_bench.json (a partial run keeps the other cases of a file already there).

Cases (seeded uniform pose vectors, D = 26 = full_body):
  a  all-vs-all full ranking + scores (stlpose::pose_rank, 2 label levels), N = 8192, every method (penalization "none")
  b  fused top-k (stlpose::pose_topk), k = 10 and 100, Q = 8192 against N = 150000 (euclidean, zero_coord)
  c  one query against N = 150000, k = 10 and 100
  d  the same work composed from torch ops on the same GPU, euclidean: torch.cdist + topk (b, c) and cdist + sort(stable) (a)
  e  the reference-semantics numpy loop (per-query Python loop over the database, pose_database.py:220-248) on 20 queries,
     extrapolated linearly to the 8192 queries of (a)
  f  full ranking + scores above the single-workgroup limit (stlpose::pose_rank_any, 2 label levels), N = 65536 and 131072,
     D = 34, euclidean / zero_coord, one batch of 256 database rows as queries (its workspace, 16 B x Q x N, is within the
     1 GiB budget of pose_database.RANK_WORKSPACE_BUDGET), against the obvious alternative on the same batch: pose_distances +
     torch.sort(stable=True) on the device + retrieval._score_rows on the host.  Host clock around work that ends in a device
     synchronise (the alternative ends on the host), the two paths alternating (20 batches of the HIP path, one of the
     alternative per sample), median of 3 samples after one warm-up of each; the
     warm-up also checks that both give the same scores.  The whole-experiment time is the batch time x N / 256, extrapolated.
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


def full_ranking(C):
    """Case f."""
    from stlpose_amd import capi
    from stlpose_amd.pose_database import RANK_WORKSPACE_BUDGET, rank_any_batch
    from stlpose_amd.retrieval import _score_rows
    d, nq = 34, 256
    for n in (65536, 131072):
        gen = torch.Generator(device="cuda").manual_seed(n)
        db = torch.rand(n, d, device="cuda", generator=gen) * 2 - 1
        lab = torch.stack([torch.randint(0, 60, (n,), device="cuda", generator=gen),
                           torch.randint(0, 8, (n,), device="cuda", generator=gen)]).to(torch.int32)
        lab_h = lab.cpu().numpy()
        assert nq <= rank_any_batch(n, nq)
        q, qlab = db[:nq], lab[:, :nq].contiguous()

        def hip():
            s = torch.ops.stlpose.pose_rank_any(q, None, db, "euclidean", "zero_coord", 0, lab, qlab, n)[2]
            return s.cpu().numpy()

        split = {}

        def composed():
            t0 = time.perf_counter()
            idx = torch.sort(torch.ops.stlpose.pose_distances(q, None, db, "euclidean", "zero_coord"), dim=1, stable=True).indices
            idx = idx.cpu().numpy()
            t1 = time.perf_counter()
            out = np.stack([_score_rows((lab_h[li][idx[:, 1:]] == lab_h[li][:nq, None]).astype(np.int64)) for li in range(2)], axis=1)
            split.setdefault("device", []).append(t1 - t0), split.setdefault("host", []).append(time.perf_counter() - t1)
            return out

        def clock(fn, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps

        a, b = hip(), composed()   # warm-up of both paths, and the check that they compute the same thing
        counts = [0, 1, 2, 3, 5, 6, 7, 8]
        same = bool(np.array_equal(a[:, :, counts], b[:, :, counts]) and np.abs(a - b).max() <= 2e-11)
        split.clear()
        th, tc = [], []
        for _ in range(3):
            th.append(clock(hip, 20)), tc.append(clock(composed, 1))   # 20 batches: the HIP path takes milliseconds
        sh, sc = float(np.median(th)), float(np.median(tc))
        C[f"f_rank_any_scores_N{n}"] = {
            "D": d, "queries_per_batch": nq, "workspace_bytes": int(capi.lib().stl_pose_rank_any_workspace(nq, n)),
            "workspace_budget_bytes": RANK_WORKSPACE_BUDGET, "seconds_per_batch": sh, "seconds_per_batch_all": th,
            "seconds_per_query": sh / nq, "seconds_whole_experiment_extrapolated": sh / nq * n,
            "scores_equal_composed": same}
        C[f"f_composed_distances_sort_hostscore_N{n}"] = {
            "D": d, "queries_per_batch": nq, "seconds_per_batch": sc, "seconds_per_batch_all": tc,
            "seconds_per_batch_device_part": float(np.median(split["device"])),
            "seconds_per_batch_host_part": float(np.median(split["host"])),
            "seconds_per_query": sc / nq, "seconds_whole_experiment_extrapolated": sc / nq * n}
        C[f"f_composed_over_rank_any_N{n}"] = sc / sh
        C[f"f_composed_device_part_over_rank_any_N{n}"] = float(np.median(split["device"])) / sh


def main(outdir, which="all"):
    if which not in ("all", "classic", "full_ranking"):
        raise SystemExit("retrieval_bench: cases are all, classic or full_ranking")
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench: no GPU")
    import stlpose_amd  # noqa: F401
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "retrieval_bench.json")
    res = {"device": torch.cuda.get_device_name(0), "D": D, "cases": {}}
    if which != "all" and os.path.exists(path):
        res = json.load(open(path))
    if which != "full_ranking":
        classic(res)
    if which != "classic":
        full_ranking(res["cases"])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def classic(res):
    """Cases a to e."""
    from stlpose_amd import capi
    import retrieval_ref as R
    gen = torch.Generator(device="cuda").manual_seed(0)
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


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        raise SystemExit("usage: retrieval_bench.py OUTDIR [all | classic | full_ranking]")
    main(*sys.argv[1:])
