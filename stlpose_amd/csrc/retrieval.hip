// Pose retrieval on gfx950: pose vectors, per-pair metrics, exact k-NN (fused distance + top-k), full ranking + scores.
// Replaces the per-query Python loops of the reference's lib/pose_database.py:19-69,149-285 and lib/metrics.py:25-149, and the
// hnswlib index of src/06_fit_knn_tree.py:150-166.
//
// Exactness contract.  Every kernel evaluates a (query, database row) pair through ONE routine, pair_dist(), so the distance of a
// pair is bit-identical in stl_pose_distances, stl_pose_topk and stl_pose_rank.  Its accumulation order is fixed: one sequential
// chain over d = 0 .. D-1 (oks: over keypoints i = 0 .. D/2-1), products folded with an explicit fmaf where written, nothing else
// contracted (fp contract is off for this file).  The result is canonicalised (-0 -> +0, every NaN -> 0x7fc00000) so that the
// order key below is a function of the value alone.
//
// Order.  A candidate is the 64-bit key (orderable bits of the distance) << 32 | database index: ascending distance, ties by
// ascending index, NaN after +inf -- the order of np.argsort(kind="stable").  Keys are unique, so any correct sort or selection on
// them is stable by construction.
#include "common.cuh"

#pragma clang fp contract(off)

namespace {

constexpr float kEps = 1e-5f;   // pose_database.py:219,239: "occluded" coordinate threshold
constexpr int kPenRows = 100;   // pose_database.py:251: rows the mean / max penalty is taken over
constexpr int kRound = 256;     // rows (or merged keys) per selection round = threads of the top-k workgroups
constexpr uint64_t kMaxKey = ~0ull;

// OKS sigmas (metrics.py:122-123, divided by 10), as 1 / (2 sigma^2) per keypoint in keypoint order 0..16: compile-time constants,
// so every device sees them without an upload
__host__ __device__ constexpr float inv2s2(double sigma) { return (float)(1.0 / ((sigma / 10.0) * (sigma / 10.0) * 2.0)); }
__constant__ const float c_inv2s2[17] = {inv2s2(.26), inv2s2(.25), inv2s2(.25), inv2s2(.35), inv2s2(.35), inv2s2(.79),
                                         inv2s2(.79), inv2s2(.72), inv2s2(.72), inv2s2(.62), inv2s2(.62), inv2s2(1.07),
                                         inv2s2(1.07), inv2s2(.87), inv2s2(.87), inv2s2(.89), inv2s2(.89)};

// keypoint i of a pose vector of dimension D (pose_database.py:35-43): all_kpts 0..16; full_body 5..16,0; upper_body 5..12,0
template <int D>
__device__ __forceinline__ int kpt_of(int i) {
    if constexpr (D == 34) return i;
    else return i == D / 2 - 1 ? 0 : 5 + i;
}

__device__ __forceinline__ float canon(float r) { return r != r ? __uint_as_float(0x7fc00000u) : (r == 0.f ? 0.f : r); }

__device__ __forceinline__ uint64_t make_key(float d, uint32_t i) {
    uint32_t b = __float_as_uint(d);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 32) | i;
}
__device__ __forceinline__ float key_dist(uint64_t k) {
    uint32_t b = (uint32_t)(k >> 32);
    b = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
    return __uint_as_float(b);
}

// Penalization as compiled: mean and max differ only in the penalty VALUE (a runtime argument), not in the per-pair masking.
enum { PZ = 0, PNONE = 1, PMM = 2 };

// THE per-pair metric.  q, c: query and its confidence (LDS broadcast); x: database row (registers); pen: mean/max penalty.
//   euclidean  sqrt(sum (q-x)^2)                      pose_database.py:202
//   cosine     1 - sum q x (vectors as given)         :200
//   manhattan  sum |q-x|                              :204
//   confidence metrics.py:97-117 as (s / sum c) * sqrt(sum c (q-x)^2 / s), s = sqrt(sum c^2): the reference's c / s folded out
//   oks        metrics.py:120-149, 1 - mean_i exp(-((dx^2 + dy^2) / (2 sigma_i^2)))
//   l2sq       hnswlib space "l2": sum (q-x)^2, unmasked
//   cos_norm   hnswlib space "cosine": 1 - (sum q x / (|q| + 1e-30)) / (|x| + 1e-30), unmasked
// Masking (pose_database.py:209-245): none: |q_d| < eps -> q_d = x_d = c_d = 0; mean/max: |q_d| < eps and |x_d| > eps -> q_d = pen,
// x_d = c_d = 0.  Not applied to l2sq / cos_norm.
template <int M, int P, int D>
__device__ __forceinline__ float pair_dist(const float* __restrict__ q, const float* __restrict__ c, const float (&x)[D], float pen) {
    constexpr bool masked = M != STL_POSE_L2SQ && M != STL_POSE_COS_NORMALISED;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    float prev = 0.f;   // oks: x-difference of the keypoint being formed
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float qd = q[d], xd = x[d], cd = (M == STL_POSE_CONFIDENCE) ? c[d] : 1.f;
        if constexpr (masked && P == PNONE) {
            if (fabsf(qd) < kEps) qd = 0.f, xd = 0.f, cd = 0.f;
        } else if constexpr (masked && P == PMM) {
            if (fabsf(qd) < kEps && fabsf(xd) > kEps) qd = pen, xd = 0.f, cd = 0.f;
        }
        if constexpr (M == STL_POSE_EUCLIDEAN || M == STL_POSE_L2SQ) {
            const float t = qd - xd;
            s0 = fmaf(t, t, s0);
        } else if constexpr (M == STL_POSE_COSINE) {
            s0 = fmaf(qd, xd, s0);
        } else if constexpr (M == STL_POSE_MANHATTAN) {
            s0 = s0 + fabsf(qd - xd);
        } else if constexpr (M == STL_POSE_CONFIDENCE) {
            const float t = qd - xd;
            s0 = fmaf(cd, t * t, s0);
            s1 = fmaf(cd, cd, s1);
            s2 = s2 + cd;
        } else if constexpr (M == STL_POSE_OKS) {
            const float t = qd - xd;
            if (d & 1) {
                const float sq = prev * prev + t * t;
                s0 = s0 + expf(-(sq * c_inv2s2[kpt_of<D>(d >> 1)]));
            } else {
                prev = t;
            }
        } else {   // STL_POSE_COS_NORMALISED
            s0 = fmaf(qd, xd, s0);
            s1 = fmaf(qd, qd, s1);
            s2 = fmaf(xd, xd, s2);
        }
    }
    float r;
    if constexpr (M == STL_POSE_EUCLIDEAN) r = sqrtf(s0);
    else if constexpr (M == STL_POSE_COSINE) r = 1.f - s0;
    else if constexpr (M == STL_POSE_MANHATTAN || M == STL_POSE_L2SQ) r = s0;
    else if constexpr (M == STL_POSE_CONFIDENCE) {
        const float s = sqrtf(s1);
        r = (s / s2) * sqrtf(s0 / s);
    } else if constexpr (M == STL_POSE_OKS) r = 1.f - s0 / (float)(D / 2);
    else r = 1.f - (s0 / (sqrtf(s1) + 1e-30f)) / (sqrtf(s2) + 1e-30f);
    return canon(r);
}

template <int D>
__device__ __forceinline__ void load_row(const float* __restrict__ db, int64_t row, float (&x)[D]) {
    const float2* p = reinterpret_cast<const float2*>(db + row * D);   // D even: rows are 8-byte aligned
#pragma unroll
    for (int i = 0; i < D / 2; ++i) {
        const float2 v = p[i];
        x[2 * i] = v.x, x[2 * i + 1] = v.y;
    }
}

// Stage nq queries (slots [0, nslot), slots >= nq zero-filled) into LDS: sq/sc [slot][DP], spen[slot].  The mean/max penalty of a
// query (pose_database.py:251-285) is the UNMASKED metric over database rows 0 .. min(100, N)-1, reduced sequentially in row order
// by one thread: every workgroup that needs it recomputes it the same way, so it is the same value in every kernel.
// tmp: >= nslot * 100 floats of scratch LDS.  Ends with a barrier.
template <int M, int P, int D, int DP>
__device__ void stage_queries(const float* __restrict__ q, const float* __restrict__ conf, const float* __restrict__ db, int N, int q0,
                              int nq, int nslot, bool is_max, float* sq, float* sc, float* spen, float* tmp) {
    for (int e = threadIdx.x; e < nslot * DP; e += blockDim.x) {
        const int j = e / DP, d = e - j * DP;
        const bool ok = j < nq && d < D;
        sq[e] = ok ? q[(int64_t)(q0 + j) * D + d] : 0.f;
        sc[e] = ok ? (conf ? conf[(int64_t)(q0 + j) * D + d] : 1.f) : 0.f;
    }
    if (threadIdx.x < nslot) spen[threadIdx.x] = 0.f;
    __syncthreads();
    if constexpr (P == PMM) {
        const int np = N < kPenRows ? N : kPenRows;
        for (int e = threadIdx.x; e < nq * np; e += blockDim.x) {
            const int j = e / np, r = e - j * np;
            float x[D];
            load_row<D>(db, r, x);
            tmp[j * kPenRows + r] = pair_dist<M, PZ, D>(sq + j * DP, sc + j * DP, x, 0.f);
        }
        __syncthreads();
        if (threadIdx.x < nq) {
            const float* t = tmp + threadIdx.x * kPenRows;
            float acc = t[0];
            for (int r = 1; r < np; ++r) {
                const float v = t[r];
                acc = is_max ? ((v != v || v > acc) ? v : acc) : acc + v;
            }
            spen[threadIdx.x] = is_max ? acc : acc / (float)np;
        }
        __syncthreads();
    }
}

// Ascending bitonic sort of n (power of two) keys in LDS by the whole workgroup.  Begins and ends with a barrier.
__device__ void bitonic_sort(uint64_t* a, int n) {
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t x = a[i], y = a[j];
                if ((x > y) == ((i & size) == 0)) a[i] = y, a[j] = x;
            }
            __syncthreads();
        }
    }
}

// Selection buffer of one query: buf[B] keys, *cnt live entries, *thr = key a candidate must beat.  Invariant: cnt + kRound <= B
// before every round.  Sort-and-truncate keeps the k smallest and raises the threshold to the k-th.
__device__ void sort_trunc(uint64_t* buf, int* cnt, uint64_t* thr, int B, int k) {
    __syncthreads();
    const int c = *cnt;
    for (int i = c + threadIdx.x; i < B; i += blockDim.x) buf[i] = kMaxKey;
    bitonic_sort(buf, B);
    if (threadIdx.x == 0 && c >= k) *cnt = k, *thr = buf[k - 1];
    __syncthreads();
}

// ---------------------------------------------------------------- pose vectors (06_fit_knn_tree.py:84-147, pose_database.py:19-69)
template <int D>
__global__ __launch_bounds__(256) void pose_vectors_kernel(const float* __restrict__ joints, int64_t stride, int C, float* __restrict__ out,
                                                           int N, int normalize) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* j = joints + (int64_t)n * stride;
    float v[D];
#pragma unroll
    for (int i = 0; i < D / 2; ++i) {
        const int k = kpt_of<D>(i);
        v[2 * i] = j[k * C], v[2 * i + 1] = j[k * C + 1];
    }
    const float ox = v[0], oy = v[1];   // the FIRST selected keypoint (nose for all_kpts, left shoulder otherwise)
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = v[d] == 0.f ? 0.f : v[d] - ((d & 1) ? oy : ox);
    if (normalize) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) s = fmaf(v[d], v[d], s);
        float nrm = sqrtf(s);
        nrm = nrm > kEps ? nrm : kEps;
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = v[d] / nrm;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) out[(int64_t)n * D + d] = v[d];
}

// ---------------------------------------------------------------- [Q,N] distance matrix: one query per workgroup row, 4 rows/thread
constexpr int kDistRows = 1024;
template <int M, int P, int D>
__global__ __launch_bounds__(256) void pose_dist_kernel(const float* __restrict__ q, const float* __restrict__ conf,
                                                        const float* __restrict__ db, float* __restrict__ out, int N, int is_max) {
    constexpr int DP = (D + 3) & ~3;
    __shared__ __attribute__((aligned(16))) float sq[DP], sc[DP], spen[1], tmp[kPenRows];
    const int qi = blockIdx.y;
    stage_queries<M, P, D, DP>(q, conf, db, N, qi, 1, 1, is_max, sq, sc, spen, tmp);
    const float pen = spen[0];
    for (int r = blockIdx.x * kDistRows + threadIdx.x; r < N && r < (blockIdx.x + 1) * kDistRows; r += blockDim.x) {
        float x[D];
        load_row<D>(db, r, x);
        out[(int64_t)qi * N + r] = pair_dist<M, P, D>(sq, sc, x, pen);
    }
}

// ---------------------------------------------------------------- fused distance + top-k
// Workgroup = 256 threads, a tile of QT queries (slots, multiple of 4) x one chunk of database rows.  Per round every thread takes
// one row (8-byte loads of its own row; the wave covers 64 consecutive rows = one contiguous span) and evaluates it against the QT
// queries read from LDS as broadcasts, four independent fmaf chains at a time.  A pair whose key beats the query's threshold is
// appended to that query's LDS buffer (LDS atomic on the count).  Before a round, a query whose buffer could overflow is sorted
// and truncated to k.  LDS: QT * B * 8 B of buffers (B = pow2 >= k + 256, QT = min(65536 / 8B, roundup4(Q)): at most 64 KiB) + QT * 2 * DP * 4 B.
// Output: the chunk's first k keys (padded with kMaxKey) into the partial list, or the final (idx, dist) when there is one chunk.
struct TopkArgs {
    const float* q;
    const float* conf;
    const float* db;
    int64_t* idx;
    float* dist;
    uint64_t* part;   // [Q][nchunk][k] keys, or NULL when nchunk == 1
    int Q, N, k, B, QT, nchunk, chunk_rows, is_max;
};

template <int M, int P, int D>
__global__ __launch_bounds__(256) void pose_topk_kernel(const TopkArgs a) {
    constexpr int DP = (D + 3) & ~3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int QT = a.QT, B = a.B, k = a.k;
    uint64_t* sbuf = reinterpret_cast<uint64_t*>(smem);   // [QT][B]
    uint64_t* sthr = sbuf + (size_t)QT * B;               // [QT]
    float* sq = reinterpret_cast<float*>(sthr + QT);      // [QT][DP]
    float* sc = sq + QT * DP;                             // [QT][DP]
    float* spen = sc + QT * DP;                           // [QT]
    int* scnt = reinterpret_cast<int*>(spen + QT);        // [QT]
    const int q0 = blockIdx.y * QT, nq = min(QT, a.Q - q0);
    const int chunk = blockIdx.x, r0 = chunk * a.chunk_rows, r1 = min(a.N, r0 + a.chunk_rows);
    stage_queries<M, P, D, DP>(a.q, a.conf, a.db, a.N, q0, nq, QT, a.is_max, sq, sc, spen, reinterpret_cast<float*>(sbuf));
    if (threadIdx.x < QT) scnt[threadIdx.x] = 0, sthr[threadIdx.x] = kMaxKey;
    __syncthreads();
    for (int base = r0; base < r1; base += kRound) {
        for (int j = 0; j < nq; ++j)
            if (scnt[j] + kRound > B) sort_trunc(sbuf + (size_t)j * B, scnt + j, sthr + j, B, k);   // uniform: LDS after a barrier
        const int row = base + threadIdx.x;
        if (row < r1) {
            float x[D];
            load_row<D>(a.db, row, x);
            for (int j = 0; j < nq; j += 4) {
                float dv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) dv[u] = pair_dist<M, P, D>(sq + (j + u) * DP, sc + (j + u) * DP, x, spen[j + u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint64_t key = make_key(dv[u], (uint32_t)row);
                    if (j + u < nq && key < sthr[j + u]) {
                        const int s = atomicAdd(scnt + j + u, 1);
                        sbuf[(size_t)(j + u) * B + s] = key;
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int j = 0; j < nq; ++j) {
        sort_trunc(sbuf + (size_t)j * B, scnt + j, sthr + j, B, k);
        const uint64_t* b = sbuf + (size_t)j * B;
        const int64_t qi = q0 + j;
        if (a.nchunk == 1) {
            for (int r = threadIdx.x; r < k; r += blockDim.x) {
                a.idx[qi * k + r] = (int64_t)(uint32_t)b[r];
                a.dist[qi * k + r] = key_dist(b[r]);
            }
        } else {
            uint64_t* o = a.part + (qi * a.nchunk + chunk) * k;
            for (int r = threadIdx.x; r < k; r += blockDim.x) o[r] = b[r];
        }
    }
}

// Merge of the per-chunk lists: one workgroup per query streams its nchunk * k keys through the same threshold + buffer selection.
__global__ __launch_bounds__(256) void pose_topk_merge_kernel(const uint64_t* __restrict__ part, int nchunk, int k, int B,
                                                              int64_t* __restrict__ idx, float* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* sbuf = reinterpret_cast<uint64_t*>(smem);
    uint64_t* sthr = sbuf + B;
    int* scnt = reinterpret_cast<int*>(sthr + 1);
    const int64_t qi = blockIdx.x;
    const int n = nchunk * k;
    const uint64_t* p = part + qi * n;
    if (threadIdx.x == 0) *scnt = 0, *sthr = kMaxKey;
    __syncthreads();
    for (int base = 0; base < n; base += kRound) {
        if (*scnt + kRound > B) sort_trunc(sbuf, scnt, sthr, B, k);
        const int e = base + threadIdx.x;
        if (e < n) {
            const uint64_t key = p[e];
            if (key < *sthr) sbuf[atomicAdd(scnt, 1)] = key;
        }
        __syncthreads();
    }
    sort_trunc(sbuf, scnt, sthr, B, k);
    for (int r = threadIdx.x; r < k; r += blockDim.x) {
        idx[qi * k + r] = (int64_t)(uint32_t)sbuf[r];
        dist[qi * k + r] = key_dist(sbuf[r]);
    }
}

// ---------------------------------------------------------------- full ranking + retrieval scores
// One workgroup (1024 threads) per query: N keys in LDS (8 B x pow2(N) <= 128 KiB), bitonic sort, first k_out written.  Scores
// (metrics.py:25-94) per label level over ranks 1 .. k_eff-1 (rank 0 dropped): thread t owns a contiguous segment of ranks, keeps
// its relevance bits in a register mask, the per-segment counts are scanned in LDS, and the fp64 sums are reduced per wave then
// across waves in wave order.
constexpr int kRankThreads = 1024;
struct RankArgs {
    const float* q;
    const float* conf;
    const float* db;
    int64_t* idx;
    float* dist;
    const int32_t* labels;    // [L][N] or NULL
    const int32_t* qlabels;   // [L][Q]
    double* scores;           // [Q][L][10]
    int Q, N, NP, k_out, L, k_eff, is_max;
};

template <int M, int P, int D>
__global__ __launch_bounds__(kRankThreads) void pose_rank_kernel(const RankArgs a) {
    constexpr int DP = (D + 3) & ~3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);   // [NP]
    float* sq = reinterpret_cast<float*>(keys + a.NP);    // [DP]
    float* sc = sq + DP;                                  // [DP]
    float* spen = sc + DP;                                // [4]
    int* scan = reinterpret_cast<int*>(spen + 4);         // [kRankThreads]
    double* red = reinterpret_cast<double*>(scan + kRankThreads);   // [16][2]
    const int qi = blockIdx.x, tid = threadIdx.x;
    // the penalty scratch (100 floats) lives in the key array before it is filled
    stage_queries<M, P, D, DP>(a.q, a.conf, a.db, a.N, qi, 1, 1, a.is_max, sq, sc, spen, reinterpret_cast<float*>(keys));
    const float pen = spen[0];
    for (int r = tid; r < a.NP; r += kRankThreads) {
        uint64_t key = kMaxKey;
        if (r < a.N) {
            float x[D];
            load_row<D>(a.db, r, x);
            key = make_key(pair_dist<M, P, D>(sq, sc, x, pen), (uint32_t)r);
        }
        keys[r] = key;
    }
    bitonic_sort(keys, a.NP);
    for (int r = tid; r < a.k_out; r += kRankThreads) {
        a.idx[(int64_t)qi * a.k_out + r] = (int64_t)(uint32_t)keys[r];
        a.dist[(int64_t)qi * a.k_out + r] = key_dist(keys[r]);
    }
    if (!a.labels) return;
    const int m = a.k_eff - 1;                          // retrievals scored: ranks 1 .. k_eff-1
    const int seg = (m + kRankThreads - 1) / kRankThreads;   // <= 16
    const int j0 = tid * seg, j1 = min(m, j0 + seg);
    const int lane = tid & 63, wave = tid >> 6;
    for (int l = 0; l < a.L; ++l) {
        const int32_t want = a.qlabels[(int64_t)l * a.Q + qi];
        const int32_t* lab = a.labels + (int64_t)l * a.N;
        uint32_t bits = 0;
        int cnt = 0;
        for (int j = j0; j < j1; ++j) {
            const bool rel = lab[(uint32_t)keys[j + 1]] == want;
            bits |= (uint32_t)rel << (j - j0);
            cnt += rel;
        }
        scan[tid] = cnt;
        __syncthreads();
        // inclusive Hillis-Steele scan of the 1024 segment counts
        for (int off = 1; off < kRankThreads; off <<= 1) {
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int nrel = scan[kRankThreads - 1];
        int cum = scan[tid] - cnt;
        double sp = 0.0, sr = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int rel = (bits >> (j - j0)) & 1;
            cum += rel;
            if (rel) sp += (double)cum / (double)(j + 1), sr += (double)cum / (double)nrel;
        }
        for (int o = 32; o > 0; o >>= 1) sp += __shfl_xor(sp, o), sr += __shfl_xor(sr, o);
        if (lane == 0) red[wave * 2] = sp, red[wave * 2 + 1] = sr;
        __syncthreads();
        if (tid == 0) {
            double* s = a.scores + ((int64_t)qi * a.L + l) * STL_POSE_NSCORES;
            if (nrel == 0) {
                for (int i = 0; i < STL_POSE_NSCORES; ++i) s[i] = -1.0;
            } else {
                double tp = 0.0, tr = 0.0;
                for (int w = 0; w < kRankThreads / 64; ++w) tp += red[w * 2], tr += red[w * 2 + 1];
                // cumulative relevant count at rank position j (0-based over the scored list): the scan of the segment holding j
                // plus the bits of that segment up to j
                auto cum_at = [&](int j) {
                    const int t = j / seg, base = t == 0 ? 0 : scan[t - 1];
                    int c = base;
                    for (int i = t * seg; i <= j; ++i) c += lab[(uint32_t)keys[i + 1]] == want;
                    return c;
                };
                const double c1 = cum_at(0), c5 = cum_at(4), c10 = cum_at(9), cr = cum_at(nrel - 1), nr = nrel;
                s[0] = c1 / 1.0, s[1] = c5 / 5.0, s[2] = c10 / 10.0, s[3] = cr / nr, s[4] = tp / nr;
                s[5] = c1 / nr, s[6] = c5 / nr, s[7] = c10 / nr, s[8] = cr / nr, s[9] = tr / nr;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- full ranking of any N: sorted runs + merge path + scores
// Above kRun rows one workgroup cannot hold a query's keys, so the ranking is built in a global workspace of two [Q][N] key arrays:
//   1. pose_run_sort_kernel, grid (chunk of kRun rows, query): the keys of the chunk, formed by the calls pose_rank_kernel makes
//      (stage_queries with the whole N, so every chunk sees the same penalty bits), bitonic-sorted in LDS; the sorted run is
//      stored at its rows' own positions [c * kRun, min(N, (c + 1) * kRun)): the last run keeps its true length.
//   2. pose_merge_kernel, ceil(log2(runs)) passes over the two arrays: runs of width W are merged in pairs (an unpaired run is the
//      pair with an empty second half: a copy).  A workgroup owns kTile consecutive output positions; since 2W is a multiple of
//      kTile a tile lies in one pair.  It finds its two input ranges by binary search on the tile's first and last diagonal, stages
//      them in LDS (kTile keys in all), ranks every staged key in the other range by binary search -- keys are unique, so rank +
//      own position is a permutation of the tile -- and stores the tile contiguously.
//   3. pose_rank_write_kernel, one workgroup per query: idx / dist of the first k_out keys and the scores, with the arithmetic of
//      pose_rank_kernel (thread t owns ranks [t * seg, (t + 1) * seg), counts scanned, fp64 sums per wave, then in wave order).
//      Segments exceed 32 ranks here, so the relevance is recomputed in the second pass instead of kept as a bit mask.
// Every summation order is fixed by (N, k_eff) alone: two runs give the same bits.
constexpr int kRun = STL_POSE_RANK_MAX;
constexpr int kTile = 2048;
constexpr int kMergeThreads = 256;
static_assert(kRun % kTile == 0, "a merge tile must not straddle two pairs of runs");

template <int M, int P, int D>
__global__ __launch_bounds__(kRankThreads) void pose_run_sort_kernel(const float* __restrict__ q, const float* __restrict__ conf,
                                                                     const float* __restrict__ db, uint64_t* __restrict__ runs, int N,
                                                                     int is_max) {
    constexpr int DP = (D + 3) & ~3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);   // [kRun]
    float* sq = reinterpret_cast<float*>(keys + kRun);    // [DP]
    float* sc = sq + DP;                                  // [DP]
    float* spen = sc + DP;                                // [4]
    const int qi = blockIdx.y, tid = threadIdx.x;
    const int r0 = blockIdx.x * kRun, n = min(kRun, N - r0);
    int NP = 128;
    while (NP < n) NP <<= 1;
    stage_queries<M, P, D, DP>(q, conf, db, N, qi, 1, 1, is_max, sq, sc, spen, reinterpret_cast<float*>(keys));
    const float pen = spen[0];
    for (int r = tid; r < NP; r += kRankThreads) {
        uint64_t key = kMaxKey;   // above every real key (an index is < 2^24): the padding sorts behind the run and is not stored
        if (r < n) {
            float x[D];
            load_row<D>(db, r0 + r, x);
            key = make_key(pair_dist<M, P, D>(sq, sc, x, pen), (uint32_t)(r0 + r));
        }
        keys[r] = key;
    }
    bitonic_sort(keys, NP);
    uint64_t* out = runs + (int64_t)qi * N + r0;
    for (int r = tid; r < n; r += kRankThreads) out[r] = keys[r];
}

// number of keys of the sorted LDS range a[0, n) below key
__device__ __forceinline__ int lower_count(const uint64_t* a, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMergeThreads) void pose_merge_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, int N,
                                                                   int W) {
    __shared__ uint64_t sin[kTile], sout[kTile];   // 32 KiB exactly: five workgroups per CU
    int* split = reinterpret_cast<int*>(sout);     // the two diagonal splits, read by every thread before sout is written
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * kTile;                   // the tile's first output position within the query (< N by the grid)
    const int base = t0 / (2 * W) * (2 * W);             // first position of the pair of runs; W <= 2^23
    const int la = min(W, N - base), lb = max(0, min(W, N - base - W));
    const uint64_t* A = src + (int64_t)blockIdx.y * N + base;
    const uint64_t* B = A + W;                           // read only when lb > 0
    const int d0 = t0 - base, d1 = min(d0 + kTile, la + lb);
    if (tid < 2) {
        // merge path: how many of the first d merged keys come from A.  lo >= d - lb and hi <= min(d, la) keep A[mid] and
        // B[d - 1 - mid] inside their runs; with lb == 0 the range is the single point d and nothing is read.
        const int d = tid ? d1 : d0;
        int lo = max(0, d - lb), hi = min(d, la);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (A[mid] < B[d - 1 - mid]) lo = mid + 1;
            else hi = mid;
        }
        split[tid] = lo;
    }
    __syncthreads();
    const int a0 = split[0], na = split[1] - a0, b0 = d0 - a0, nt = d1 - d0, nb = nt - na;   // na + nb = nt <= kTile
    for (int e = tid; e < nt; e += kMergeThreads) sin[e] = e < na ? A[a0 + e] : B[b0 + (e - na)];
    __syncthreads();
    for (int e = tid; e < nt; e += kMergeThreads) {
        const uint64_t key = sin[e];
        const int pos = e < na ? e + lower_count(sin + na, nb, key) : (e - na) + lower_count(sin, na, key);
        sout[pos] = key;
    }
    __syncthreads();
    uint64_t* o = dst + (int64_t)blockIdx.y * N + t0;
    for (int e = tid; e < nt; e += kMergeThreads) o[e] = sout[e];
}

struct RankWriteArgs {
    const uint64_t* keys;     // [Q][N] sorted
    int64_t* idx;
    float* dist;
    const int32_t* labels;    // [L][N] or NULL
    const int32_t* qlabels;   // [L][Q]
    double* scores;           // [Q][L][10]
    int Q, N, k_out, L, k_eff;
};

__global__ __launch_bounds__(kRankThreads) void pose_rank_write_kernel(const RankWriteArgs a) {
    __shared__ int scan[kRankThreads];
    __shared__ double red[kRankThreads / 64 * 2];
    const int qi = blockIdx.x, tid = threadIdx.x;
    const uint64_t* keys = a.keys + (int64_t)qi * a.N;
    for (int r = tid; r < a.k_out; r += kRankThreads) {
        const uint64_t key = keys[r];
        a.idx[(int64_t)qi * a.k_out + r] = (int64_t)(uint32_t)key;
        a.dist[(int64_t)qi * a.k_out + r] = key_dist(key);
    }
    if (!a.labels) return;
    const int m = a.k_eff - 1;                               // retrievals scored: ranks 1 .. k_eff-1
    const int seg = (m + kRankThreads - 1) / kRankThreads;   // <= 2^14
    const int j0 = min(m, tid * seg), j1 = min(m, j0 + seg);
    const int lane = tid & 63, wave = tid >> 6;
    for (int l = 0; l < a.L; ++l) {
        const int32_t want = a.qlabels[(int64_t)l * a.Q + qi];
        const int32_t* lab = a.labels + (int64_t)l * a.N;
        int cnt = 0;
        for (int j = j0; j < j1; ++j) cnt += lab[(uint32_t)keys[j + 1]] == want;
        scan[tid] = cnt;
        __syncthreads();
        for (int off = 1; off < kRankThreads; off <<= 1) {
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int nrel = scan[kRankThreads - 1];
        int cum = scan[tid] - cnt;
        double sp = 0.0, sr = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int rel = lab[(uint32_t)keys[j + 1]] == want;
            cum += rel;
            if (rel) sp += (double)cum / (double)(j + 1), sr += (double)cum / (double)nrel;
        }
        for (int o = 32; o > 0; o >>= 1) sp += __shfl_xor(sp, o), sr += __shfl_xor(sr, o);
        if (lane == 0) red[wave * 2] = sp, red[wave * 2 + 1] = sr;
        __syncthreads();
        if (tid == 0) {
            double* s = a.scores + ((int64_t)qi * a.L + l) * STL_POSE_NSCORES;
            if (nrel == 0) {
                for (int i = 0; i < STL_POSE_NSCORES; ++i) s[i] = -1.0;
            } else {
                double tp = 0.0, tr = 0.0;
                for (int w = 0; w < kRankThreads / 64; ++w) tp += red[w * 2], tr += red[w * 2 + 1];
                auto cum_at = [&](int j) {   // relevant among scored positions 0 .. j: the scan up to j's segment plus a recount
                    const int t = j / seg;
                    int c = t == 0 ? 0 : scan[t - 1];
                    for (int i = t * seg; i <= j; ++i) c += lab[(uint32_t)keys[i + 1]] == want;
                    return c;
                };
                const double c1 = cum_at(0), c5 = cum_at(4), c10 = cum_at(9), cr = cum_at(nrel - 1), nr = nrel;
                s[0] = c1 / 1.0, s[1] = c5 / 5.0, s[2] = c10 / 10.0, s[3] = cr / nr, s[4] = tp / nr;
                s[5] = c1 / nr, s[6] = c5 / nr, s[7] = c10 / nr, s[8] = cr / nr, s[9] = tr / nr;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- dispatch over (method, penalization, D)
static int check_common(int D, int method, int pen) {
    STL_CHECK(D == 18 || D == 26 || D == 34, "pose: D = %d (pose vectors have 18, 26 or 34 entries)", D);
    STL_CHECK(method >= 0 && method <= STL_POSE_COS_NORMALISED, "pose: unknown method %d", method);
    STL_CHECK(pen >= 0 && pen <= STL_POSE_PEN_MAX, "pose: unknown penalization %d", pen);
    return 0;
}

static int pen_class(int method, int pen) {
    if (method == STL_POSE_L2SQ || method == STL_POSE_COS_NORMALISED) return PZ;
    return pen == STL_POSE_PEN_ZERO_COORD ? PZ : pen == STL_POSE_PEN_NONE ? PNONE : PMM;
}

// F<M, P, D>() for the runtime triple; F is a generic lambda taking three integral_constants
template <typename F>
static void dispatch(int method, int pen, int D, F&& f) {
    auto byD = [&](auto m, auto p) {
        if (D == 18) f(m, p, std::integral_constant<int, 18>{});
        else if (D == 26) f(m, p, std::integral_constant<int, 26>{});
        else f(m, p, std::integral_constant<int, 34>{});
    };
    auto byP = [&](auto m) {
        const int pc = pen_class(method, pen);
        if constexpr (decltype(m)::value == STL_POSE_L2SQ || decltype(m)::value == STL_POSE_COS_NORMALISED) {
            byD(m, std::integral_constant<int, PZ>{});
        } else {
            if (pc == PZ) byD(m, std::integral_constant<int, PZ>{});
            else if (pc == PNONE) byD(m, std::integral_constant<int, PNONE>{});
            else byD(m, std::integral_constant<int, PMM>{});
        }
    };
    switch (method) {
        case STL_POSE_EUCLIDEAN: byP(std::integral_constant<int, STL_POSE_EUCLIDEAN>{}); break;
        case STL_POSE_COSINE: byP(std::integral_constant<int, STL_POSE_COSINE>{}); break;
        case STL_POSE_MANHATTAN: byP(std::integral_constant<int, STL_POSE_MANHATTAN>{}); break;
        case STL_POSE_CONFIDENCE: byP(std::integral_constant<int, STL_POSE_CONFIDENCE>{}); break;
        case STL_POSE_OKS: byP(std::integral_constant<int, STL_POSE_OKS>{}); break;
        case STL_POSE_L2SQ: byP(std::integral_constant<int, STL_POSE_L2SQ>{}); break;
        default: byP(std::integral_constant<int, STL_POSE_COS_NORMALISED>{}); break;
    }
}

struct TopkPlan {
    int B, QT, nchunk, chunk_rows;
};
static TopkPlan topk_plan(int Q, int N, int k) {
    TopkPlan p;
    p.B = 512;
    while (p.B < k + kRound) p.B <<= 1;
    p.QT = 65536 / (p.B * 8);                 // 16 / 8 / 4 query slots for B = 512 / 1024 / 2048: 64 KiB of buffers
    const int q4 = (Q + 3) & ~3;              // slots are evaluated four at a time: a small Q needs no more than roundup4(Q)
    p.QT = q4 < p.QT ? q4 : p.QT;
    const int qtiles = ceil_div(Q, p.QT);
    const int want = ceil_div(1024, qtiles);   // ~4 workgroups per CU over 256 CUs
    const int maxc = N / 2048 > 1 ? N / 2048 : 1;
    p.nchunk = want < maxc ? want : maxc;
    p.chunk_rows = ceil_div(ceil_div(N, p.nchunk), kRound) * kRound;
    p.nchunk = ceil_div(N, p.chunk_rows);
    return p;
}
static size_t topk_lds(const TopkPlan& p, int D) {
    const int DP = (D + 3) & ~3;
    return (size_t)p.QT * p.B * 8 + p.QT * 8 + (size_t)p.QT * 2 * DP * 4 + p.QT * 4 + p.QT * 4;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_pose_vectors(const float* joints, int64_t row_stride, int C, float* out, int N, int approach, int normalize,
                                void* stream) {
    STL_CHECK(approach >= STL_POSE_ALL_KPTS && approach <= STL_POSE_UPPER_BODY, "pose_vectors: unknown approach %d", approach);
    STL_CHECK(C >= 2 && row_stride >= 17 * C && N >= 0, "pose_vectors: joints must be [N,17,C>=2] (C=%d, row stride %lld)", C,
              (long long)row_stride);
    if (N == 0) return 0;
    STL_CHECK(joints && out, "pose_vectors: null pointer");
    const dim3 g(ceil_div(N, 256)), b(256);
    if (approach == STL_POSE_ALL_KPTS) STL_LAUNCH(pose_vectors_kernel<34>, g, b, 0, ST, joints, row_stride, C, out, N, normalize);
    else if (approach == STL_POSE_FULL_BODY) STL_LAUNCH(pose_vectors_kernel<26>, g, b, 0, ST, joints, row_stride, C, out, N, normalize);
    else STL_LAUNCH(pose_vectors_kernel<18>, g, b, 0, ST, joints, row_stride, C, out, N, normalize);
    STL_LAUNCH_CHECK("pose_vectors");
    return 0;
}

extern "C" int stl_pose_distances(const float* q, const float* conf, const float* db, float* out, int Q, int N, int D, int method,
                                  int penalization, void* stream) {
    if (int rc = check_common(D, method, penalization)) return rc;
    STL_CHECK(Q >= 0 && N >= 0 && Q <= 65535, "pose_distances: Q = %d, N = %d (Q <= 65535 per call)", Q, N);
    if (Q == 0 || N == 0) return 0;
    STL_CHECK(q && db && out, "pose_distances: null pointer");
    const int is_max = penalization == STL_POSE_PEN_MAX;
    dispatch(method, penalization, D, [&](auto m, auto p, auto d) {
        STL_LAUNCH((pose_dist_kernel<decltype(m)::value, decltype(p)::value, decltype(d)::value>), dim3(ceil_div(N, kDistRows), Q),
                   dim3(256), 0, ST, q, conf, db, out, N, is_max);
    });
    STL_LAUNCH_CHECK("pose_distances");
    return 0;
}

extern "C" int stl_pose_topk_workspace(int Q, int N, int k, int D) {
    STL_CHECK(Q >= 0 && N >= 1 && k >= 1 && k <= STL_POSE_TOPK_MAX && k <= N, "pose_topk: k = %d with N = %d (1 <= k <= min(N, %d))",
              k, N, STL_POSE_TOPK_MAX);
    (void)D;
    if (Q == 0) return 0;
    const TopkPlan p = topk_plan(Q, N, k);
    const size_t bytes = p.nchunk == 1 ? 0 : (size_t)Q * p.nchunk * k * 8;
    STL_CHECK(bytes < (1ull << 31), "pose_topk: workspace of %zu bytes", bytes);
    return (int)bytes;
}

extern "C" int stl_pose_topk(const float* q, const float* conf, const float* db, int Q, int N, int D, int method, int penalization,
                             int k, int64_t* idx, float* dist, void* work, int64_t work_bytes, void* stream) {
    if (int rc = check_common(D, method, penalization)) return rc;
    const int need = stl_pose_topk_workspace(Q, N, k, D);
    if (need < 0) return need;
    if (Q == 0) return 0;
    STL_CHECK(q && db && idx && dist, "pose_topk: null pointer");
    STL_CHECK(work_bytes >= need && (need == 0 || work), "pose_topk: workspace of %lld bytes, %d needed", (long long)work_bytes, need);
    const TopkPlan p = topk_plan(Q, N, k);
    STL_CHECK(ceil_div(Q, p.QT) <= 65535, "pose_topk: Q = %d (at most %d per call at k = %d)", Q, 65535 * p.QT, k);
    TopkArgs a{q, conf, db, idx, dist, (uint64_t*)work, Q, N, k, p.B, p.QT, p.nchunk, p.chunk_rows, penalization == STL_POSE_PEN_MAX};
    const size_t lds = topk_lds(p, D);
    dispatch(method, penalization, D, [&](auto m, auto pp, auto d) {
        auto* kern = &pose_topk_kernel<decltype(m)::value, decltype(pp)::value, decltype(d)::value>;
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        STL_LAUNCH(kern, dim3(p.nchunk, ceil_div(Q, p.QT)), dim3(256), lds, ST, a);
    });
    STL_LAUNCH_CHECK("pose_topk");
    if (p.nchunk > 1) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&pose_topk_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
        STL_LAUNCH(pose_topk_merge_kernel, dim3(Q), dim3(256), (size_t)p.B * 8 + 16, ST, (const uint64_t*)work, p.nchunk, k, p.B,
                   idx, dist);
        STL_LAUNCH_CHECK("pose_topk_merge");
    }
    return 0;
}

extern "C" int stl_pose_rank(const float* q, const float* conf, const float* db, int Q, int N, int D, int method, int penalization,
                             int k_out, int64_t* idx, float* dist, const int32_t* labels, const int32_t* qlabels, int L, int k_eff,
                             double* scores, void* stream) {
    if (int rc = check_common(D, method, penalization)) return rc;
    STL_CHECK(N >= 1 && N <= STL_POSE_RANK_MAX, "pose_rank: N = %d (a full ranking takes 1 <= N <= %d; use top-k above)", N,
              STL_POSE_RANK_MAX);
    STL_CHECK(Q >= 0 && k_out >= 0 && k_out <= N, "pose_rank: k_out = %d with N = %d", k_out, N);
    if (labels) {
        STL_CHECK(qlabels && scores && L >= 1 && L <= STL_POSE_RANK_LABELS_MAX, "pose_rank: scores need qlabels, scores and 1 <= L <= %d",
                  STL_POSE_RANK_LABELS_MAX);
        STL_CHECK(k_eff >= 11 && k_eff <= N, "pose_rank: scores need 11 <= k_eff <= N (k_eff = %d, N = %d): p@10 reads rank 10", k_eff, N);
    }
    if (Q == 0) return 0;
    STL_CHECK(q && db && (k_out == 0 || (idx && dist)), "pose_rank: null pointer");
    int NP = 128;
    while (NP < N) NP <<= 1;
    const int DP = (D + 3) & ~3;
    const size_t lds = (size_t)NP * 8 + 2 * DP * 4 + 16 + kRankThreads * 4 + 16 * 2 * 8;
    RankArgs a{q, conf, db, idx, dist, labels, qlabels, scores, Q, N, NP, k_out, labels ? L : 0, k_eff, penalization == STL_POSE_PEN_MAX};
    dispatch(method, penalization, D, [&](auto m, auto pp, auto d) {
        auto* kern = &pose_rank_kernel<decltype(m)::value, decltype(pp)::value, decltype(d)::value>;
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        STL_LAUNCH(kern, dim3(Q), dim3(kRankThreads), lds, ST, a);
    });
    STL_LAUNCH_CHECK("pose_rank");
    return 0;
}

extern "C" int64_t stl_pose_rank_any_workspace(int Q, int N) {
    STL_CHECK(Q >= 0 && N >= 1 && N <= STL_POSE_RANK_ANY_MAX, "pose_rank_any: Q = %d, N = %d (a ranking takes 1 <= N <= %d)", Q, N,
              STL_POSE_RANK_ANY_MAX);
    if (N <= kRun || Q == 0) return 16;   // nothing is merged: a token size, so that every (Q, N) has a buffer
    return (int64_t)Q * N * 16;           // two [Q][N] arrays of 8-byte keys
}

extern "C" int stl_pose_rank_any(const float* q, const float* conf, const float* db, int Q, int N, int D, int method, int penalization,
                                 int k_out, int64_t* idx, float* dist, const int32_t* labels, const int32_t* qlabels, int L, int k_eff,
                                 double* scores, void* work, int64_t work_bytes, void* stream) {
    if (int rc = check_common(D, method, penalization)) return rc;
    STL_CHECK(N >= 1 && N <= STL_POSE_RANK_ANY_MAX, "pose_rank_any: N = %d (a ranking takes 1 <= N <= %d)", N, STL_POSE_RANK_ANY_MAX);
    STL_CHECK(Q >= 0 && k_out >= 0 && k_out <= N, "pose_rank_any: k_out = %d with N = %d", k_out, N);
    if (labels) {
        STL_CHECK(qlabels && scores && L >= 1 && L <= STL_POSE_RANK_LABELS_MAX,
                  "pose_rank_any: scores need qlabels, scores and 1 <= L <= %d", STL_POSE_RANK_LABELS_MAX);
        STL_CHECK(k_eff >= 11 && k_eff <= N, "pose_rank_any: scores need 11 <= k_eff <= N (k_eff = %d, N = %d): p@10 reads rank 10",
                  k_eff, N);
    }
    if (Q == 0) return 0;
    STL_CHECK(q && db && (k_out == 0 || (idx && dist)), "pose_rank_any: null pointer");
    const int64_t need = stl_pose_rank_any_workspace(Q, N);
    STL_CHECK(work && work_bytes >= need, "pose_rank_any: workspace of %lld bytes, %lld needed", (long long)(work ? work_bytes : 0),
              (long long)need);
    if (N <= kRun) return stl_pose_rank(q, conf, db, Q, N, D, method, penalization, k_out, idx, dist, labels, qlabels, L, k_eff, scores,
                                        stream);
    STL_CHECK(Q <= 65535, "pose_rank_any: Q = %d (at most 65535 queries per call above N = %d)", Q, kRun);
    STL_CHECK(((uintptr_t)work & 7) == 0, "pose_rank_any: workspace must be 8-byte aligned");
    uint64_t* buf[2] = {(uint64_t*)work, (uint64_t*)work + (int64_t)Q * N};
    const int is_max = penalization == STL_POSE_PEN_MAX;
    const int DP = (D + 3) & ~3;
    const size_t lds = (size_t)kRun * 8 + 2 * DP * 4 + 16;
    dispatch(method, penalization, D, [&](auto m, auto pp, auto d) {
        auto* kern = &pose_run_sort_kernel<decltype(m)::value, decltype(pp)::value, decltype(d)::value>;
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        STL_LAUNCH(kern, dim3(ceil_div(N, kRun), Q), dim3(kRankThreads), lds, ST, q, conf, db, buf[0], N, is_max);
    });
    STL_LAUNCH_CHECK("pose_run_sort");
    int cur = 0;
    for (int W = kRun; W < N; W <<= 1, cur ^= 1) {   // W <= 2^23: the loop ends before W could overflow
        STL_LAUNCH(pose_merge_kernel, dim3(ceil_div(N, kTile), Q), dim3(kMergeThreads), 0, ST, (const uint64_t*)buf[cur], buf[cur ^ 1], N,
                   W);
        STL_LAUNCH_CHECK("pose_merge");
    }
    RankWriteArgs a{buf[cur], idx, dist, labels, qlabels, scores, Q, N, k_out, labels ? L : 0, k_eff};
    STL_LAUNCH(pose_rank_write_kernel, dim3(Q), dim3(kRankThreads), 0, ST, a);
    STL_LAUNCH_CHECK("pose_rank_write");
    return 0;
}
