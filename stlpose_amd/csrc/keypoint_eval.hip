// Pose scoring on gfx950: what src/03_evaluate.py does after the network (lib/metrics.py:211-262 with lib/nms.py, and
// pycocotools' COCOeval(..., "keypoints"), whose published algorithm this file restates).
//
//   stl_pose_rescore_nms  one workgroup per image: score = box score x mean confidence of the confident joints (by default in
//                         numpy's own summation order, so that it equals the host function's conf[good].mean() bit for bit;
//                         on request as one running sum, which is the reference's loop bit for bit), then the greedy OKS suppression
//                         of oks_nms: the persons sorted once, and per kept person one parallel row of OKS values over the
//                         candidates still alive behind it.  No OKS matrix is stored: LDS holds the sort keys and one flag per person.
//   stl_oks_ap_match      COCOeval.evaluateImg for iouType "keypoints": one workgroup per image sorts the image's detections
//                         (stable, descending fp64 score, the first STL_OKS_AP_DETS kept), computes their OKS with the image's
//                         ground truth as computeOks does and runs the greedy match for every (threshold, area range).  Its slots
//                         have the layout of stl_box_ap_match (both end in greedy_match of coco_match.inc), so stl_box_ap_accumulate (box_ap.hip) finishes the job.
//
// Exactness.  fp contract is off for this file and every operation is fp64 in the order the host code writes it, so everything
// except exp is reproducible bit for bit.  The device's fp64 exp, and hence the sum of up to 17 of them, need not equal numpy's to
// the last bit: one OKS is a mean of at most 17 terms in [0, 1], each within an ulp or two, so the two differ by less than 1e-13.
// Matching and suppression only COMPARE OKS values (with a threshold, and with each other for the best match): the results are
// those of the host whenever no such comparison is closer than that.  Scores, ranks, counts, precision and recall are exact.
#include "common.cuh"

#pragma clang fp contract(off)

#include "coco_match.inc"

namespace {

constexpr int kJ = STL_POSE_JOINTS;
constexpr int kT = STL_OKS_AP_THRS, kA = STL_OKS_AP_AREAS;   // 30 chains
constexpr int kDets = STL_OKS_AP_DETS;
static_assert(kJ == 17, "the joint count is fixed");

// numpy's add.reduce over the values v[k] with bit k of mask set, in index order (pairwise sum below its block size): n < 8 a running
// sum from 0; else eight running sums over the first 8 * (n / 8), combined pairwise, then the rest in order.  Static indices only.
template <typename T>
__device__ __forceinline__ T numpy_sum(const T (&v)[kJ], uint32_t mask, int n, bool serial = false) {
#pragma clang fp contract(off)
    const int nb = n & ~7;
    T r[8], res = (T)0;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (T)0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kJ; ++k) {
        if (!((mask >> k) & 1)) continue;
        if (n < 8 || serial) {
            res += v[k];
        } else if (c < nb) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((c & 7) == j) r[j] += v[k];
        } else {
            if (c == nb) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            res += v[k];
        }
        ++c;
    }
    if (n >= 8 && nb == n && !serial) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    return res;
}

// ------------------------------------------------------------------------------------------------ rescoring + OKS-NMS
struct NmsArgs {
    const void* preds;        // [P, 17, 3]
    const double* boxes;      // [P, 6]
    const int64_t* offsets;   // [I + 1]
    int64_t P;
    int max_n, key_cap, serial_sum;
    double in_vis_thr, oks_thr, var[kJ];
    double* score;            // [P]
    int32_t* keep;            // [P]
    int32_t* count;           // [I]
};

// conf[good].mean() of one person in the dtype of preds, as a double; 0 without a confident joint
template <typename T>
__device__ __forceinline__ double mean_confidence(const T* p, T thr, bool serial) {
    T v[kJ];
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < kJ; ++k) {
        v[k] = p[3 * k + 2];
        mask |= (v[k] > thr ? 1u : 0u) << k;
    }
    const int n = __popc(mask);
    if (n == 0) return 0.0;
    // a quotient of a 24-bit value by n <= 17 rounded to 53 bits and then to 24 is the correctly rounded fp32 quotient
    return (double)(T)((double)numpy_sum<T>(v, mask, n, serial) / (double)n);
}

// OKS of oks_iou between the kept person (row i, area ai) and the candidate (row j, area aj), all 17 joints
template <typename T>
__device__ __forceinline__ double nms_oks(const T* pi, const T* pj, double ai, double aj, const double* var) {
#pragma clang fp contract(off)
    const double den = (ai + aj) / 2 + 0x1p-52;
    double v[kJ];
#pragma unroll
    for (int k = 0; k < kJ; ++k) {
        const double dx = (double)pj[3 * k] - (double)pi[3 * k], dy = (double)pj[3 * k + 1] - (double)pi[3 * k + 1];
        const double e = (dx * dx + dy * dy) / var[k] / den / 2;
        v[k] = exp(-e);
    }
    return numpy_sum<double>(v, (1u << kJ) - 1, kJ) / (double)kJ;
}

// LDS: skey [key_cap] u64 | sidx [key_cap] u32 | sgone [max_n] u8
template <typename T>
__global__ __launch_bounds__(kThreads) void pose_rescore_nms_kernel(const NmsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* skey = reinterpret_cast<uint64_t*>(smem);
    uint32_t* sidx = reinterpret_cast<uint32_t*>(skey + a.key_cap);
    uint8_t* sgone = reinterpret_cast<uint8_t*>(sidx + a.key_cap);

    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int64_t o0 = a.offsets[img], o1 = a.offsets[img + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.P || o1 - o0 > a.max_n) {   // refused: the wrapper checks first
        if (tid == 0) a.count[img] = -1;
        return;
    }
    const int n = (int)(o1 - o0);
    const T* preds = static_cast<const T*>(a.preds) + o0 * (kJ * 3);
    const double* boxes = a.boxes + o0 * 6;

    // 1. the scores, and the sort keys: descending score, equal scores in descending input position
    for (int r = tid; r < n; r += kThreads) {
        const double s = mean_confidence<T>(preds + (size_t)r * (kJ * 3), (T)a.in_vis_thr, a.serial_sum != 0) * boxes[r * 6 + 5];
        a.score[o0 + r] = s;
        skey[r] = ~score_bits(s), sidx[r] = (uint32_t)(n - 1 - r);
        sgone[r] = 0;
    }
    bitonic_sort<true>(skey, sidx, n, tid);

    // 2. the greedy suppression: position i is kept unless an earlier kept one took it; then its row over the positions behind it
    for (int i = 0; i < n; ++i) {
        if (sgone[i]) continue;   // the same for every thread: written before the last barrier
        const int ri = n - 1 - (int)sidx[i];
        const double ai = boxes[ri * 6 + 4];
        const T* pi = preds + (size_t)ri * (kJ * 3);
        for (int j = i + 1 + tid; j < n; j += kThreads) {
            if (sgone[j]) continue;
            const int rj = n - 1 - (int)sidx[j];
            const double v = nms_oks<T>(pi, preds + (size_t)rj * (kJ * 3), ai, boxes[rj * 6 + 4], a.var);
            if (!(v <= a.oks_thr)) sgone[j] = 1;   // as `ov <= thresh` keeps: a NaN goes
        }
        __syncthreads();
    }

    // 3. the kept rows in that order, then -1 (wave 0, 64 positions at a time)
    if (tid < 64) {
        int cnt = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            const bool is = p < n && !sgone[p];
            const uint64_t mask = __ballot(is);
            if (is) a.keep[o0 + cnt + __popcll(mask & ((1ull << lane) - 1))] = n - 1 - (int)sidx[p];
            cnt += __popcll(mask);
        }
        for (int p = cnt + lane; p < n; p += 64) a.keep[o0 + p] = -1;
        if (lane == 0) a.count[img] = cnt;
    }
}

// ------------------------------------------------------------------------------------------------ keypoint AP match
struct MatchArgs : MatchBase<kT, kA, double> {
    const double* kpts;          // [N, 17, 3]
    const double* area;          // [N] or null
    const double* gt_kpts;       // [G, 17, 3]
    const double* gt_area;       // [G]
    const double* gt_bbox;       // [G, 4] xywh
    const uint8_t* gt_crowd;     // [G]
    const int32_t* gt_numkp;     // [G]
    double var[kJ];
};

// computeOks for one (detection, ground truth) pair
__device__ __forceinline__ double ap_oks(const double* d, const double* g, const double* bb, double garea, const double* var) {
#pragma clang fp contract(off)
    uint32_t vis = 0;
#pragma unroll
    for (int k = 0; k < kJ; ++k) vis |= (g[3 * k + 2] > 0 ? 1u : 0u) << k;
    const int k1 = __popc(vis);
    const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2;
    const double den = garea + 0x1p-52;
    double v[kJ];
#pragma unroll
    for (int k = 0; k < kJ; ++k) {
        const double xd = d[3 * k], yd = d[3 * k + 1];
        double dx, dy;
        if (k1 > 0) {
            dx = xd - g[3 * k], dy = yd - g[3 * k + 1];
        } else {   // no labelled joint: the distance to the doubled box
            const double ax = x0 - xd, bx = xd - x1, ay = y0 - yd, by = yd - y1;
            dx = (ax > 0 ? ax : 0.0) + (bx > 0 ? bx : 0.0);
            dy = (ay > 0 ? ay : 0.0) + (by > 0 ? by : 0.0);
        }
        const double e = (dx * dx + dy * dy) / var[k] / den / 2;
        v[k] = exp(-e);
    }
    const uint32_t mask = k1 > 0 ? vis : (1u << kJ) - 1;
    const int n = k1 > 0 ? k1 : kJ;
    return numpy_sum<double>(v, mask, n) / (double)n;
}

// LDS: skey [key_cap] u64 | soks [kDets * max_g] f64 | sgarea [max_g] f64 | sdarea [kDets] f64 | sidx [key_cap] u32
//      | sgord [kA * max_g] u8 | sgcrowd [max_g] u8 | sgign [max_g] u8
__global__ __launch_bounds__(kThreads) void oks_ap_match_kernel(const MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int mg = a.max_g;
    uint64_t* skey = reinterpret_cast<uint64_t*>(smem);
    double* soks = reinterpret_cast<double*>(skey + a.key_cap);
    double* sgarea = soks + (size_t)kDets * mg;
    double* sdarea = sgarea + mg;
    uint32_t* sidx = reinterpret_cast<uint32_t*>(sdarea + kDets);
    uint8_t* sgord = reinterpret_cast<uint8_t*>(sidx + a.key_cap);
    uint8_t* sgcrowd = sgord + kA * mg;
    uint8_t* sgign = sgcrowd + mg;
    __shared__ int s_npig[kA];

    const int img = blockIdx.x, tid = threadIdx.x;
    int32_t* npig_out = a.npig + (size_t)img * kA;
    const int64_t o0 = a.det_offsets[img], o1 = a.det_offsets[img + 1];
    const int64_t g0 = a.gt_offsets[img], g1 = a.gt_offsets[img + 1];
    if (offsets_refused(a, o0, o1, g0, g1) || g1 - g0 > mg) {   // the wrapper checks first
        if (tid < kA) npig_out[tid] = -1;
        return;
    }
    const int m = (int)(o1 - o0), ng = (int)(g1 - g0);

    // 1. stable sort by descending score: the image-local row breaks ties
    for (int r = tid; r < m; r += kThreads) skey[r] = ~score_bits(a.scores[o0 + r]), sidx[r] = (uint32_t)r;
    // 2. the ground truth's flags
    for (int g = tid; g < ng; g += kThreads) {
        sgarea[g] = a.gt_area[g0 + g];
        sgcrowd[g] = a.gt_crowd[g0 + g] != 0;
        sgign[g] = a.gt_crowd[g0 + g] != 0 || a.gt_numkp[g0 + g] == 0;
    }
    bitonic_sort<true>(skey, sidx, m, tid);
    const int nd = m < kDets ? m : kDets;

    // 3. the kept detections' areas
    for (int d = tid; d < nd; d += kThreads) {
        const int64_t row = o0 + sidx[d];
        double ar;
        if (a.area) {
            ar = a.area[row];
        } else {
            const double* p = a.kpts + row * (kJ * 3);
            double xmin = p[0], xmax = p[0], ymin = p[1], ymax = p[1];
#pragma unroll
            for (int k = 1; k < kJ; ++k) {
                const double x = p[3 * k], y = p[3 * k + 1];
                xmin = x < xmin ? x : xmin, xmax = x > xmax ? x : xmax;
                ymin = y < ymin ? y : ymin, ymax = y > ymax ? y : ymax;
            }
            ar = (xmax - xmin) * (ymax - ymin);
        }
        sdarea[d] = ar;
    }
    // 4. the ground truth in each area range's order (ignored: a crowd, no labelled joint, or outside the range)
    order_ground_truth(a, sgign, sgarea, ng, sgord, s_npig, npig_out, tid);
    // 5. the OKS tile, fp64
    for (int e = tid; e < nd * ng; e += kThreads) {
        const int d = e / ng, g = e - d * ng;
        soks[e] = ap_oks(a.kpts + (o0 + sidx[d]) * (kJ * 3), a.gt_kpts + (g0 + g) * (kJ * 3), a.gt_bbox + (g0 + g) * 4, sgarea[g], a.var);
    }
    __syncthreads();
    if (tid >= 64) return;

    // 6. the greedy match
    greedy_match(a, soks, sgcrowd, sgord, s_npig, nd, ng, o0, o0, 0, [&](int d) { return sdarea[d]; }, [&](int d) { return sidx[d]; }, tid);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_pose_rescore_nms(const void* preds, int preds_f64, int sum_order, const double* boxes, const int64_t* offsets, int num_images,
                                    int64_t P, int max_n, double in_vis_thr, double oks_thr, const double* var, double* score,
                                    int32_t* keep, int32_t* count, void* stream) {
    STL_CHECK(num_images >= 0 && P >= 0 && P < (1ll << 31), "pose_rescore_nms: %d images, P = %lld", num_images, (long long)P);
    STL_CHECK(preds_f64 == 0 || preds_f64 == 1, "pose_rescore_nms: preds_f64 = %d (0 or 1)", preds_f64);
    STL_CHECK(sum_order == STL_POSE_SUM_NUMPY || sum_order == STL_POSE_SUM_SERIAL, "pose_rescore_nms: sum_order = %d (0 or 1)", sum_order);
    STL_CHECK(max_n >= 0 && max_n <= STL_POSE_NMS_MAX, "pose_rescore_nms: max_n = %d (at most %d persons per image)", max_n,
              STL_POSE_NMS_MAX);
    STL_CHECK(var, "pose_rescore_nms: null var");
    if (num_images == 0) return 0;
    STL_CHECK(offsets && count, "pose_rescore_nms: null pointer");
    STL_CHECK(P == 0 || (preds && boxes && score && keep), "pose_rescore_nms: null person pointer");
    NmsArgs a{};
    a.preds = preds, a.boxes = boxes, a.offsets = offsets, a.P = P, a.max_n = max_n, a.key_cap = pow2_at_least(max_n > 0 ? max_n : 1);
    a.in_vis_thr = in_vis_thr, a.oks_thr = oks_thr, a.serial_sum = sum_order == STL_POSE_SUM_SERIAL;
    for (int k = 0; k < kJ; ++k) a.var[k] = var[k];
    a.score = score, a.keep = keep, a.count = count;
    const size_t lds = (size_t)a.key_cap * 12 + (size_t)(max_n > 0 ? max_n : 1);   // 13 KiB at the cap
    for (int i0 = 0; i0 < num_images; i0 += 1 << 20) {   // grid.x is the image: any number of them
        NmsArgs b = a;
        const int ni = num_images - i0 < (1 << 20) ? num_images - i0 : (1 << 20);
        b.offsets += i0, b.count += i0;
        if (preds_f64) STL_LAUNCH(pose_rescore_nms_kernel<double>, dim3(ni), dim3(kThreads), lds, ST, b);
        else STL_LAUNCH(pose_rescore_nms_kernel<float>, dim3(ni), dim3(kThreads), lds, ST, b);
        STL_LAUNCH_CHECK("pose_rescore_nms");
    }
    return 0;
}

extern "C" int stl_oks_ap_match(const double* kpts, const double* scores, const double* area, const int64_t* det_offsets, int64_t N,
                                int max_n, const double* gt_kpts, const double* gt_area, const double* gt_bbox, const uint8_t* gt_crowd,
                                const int32_t* gt_numkp, const int64_t* gt_offsets, int64_t G, int max_g, int num_images,
                                const double* oks_thrs, const double* area_ranges, const double* var, double* slot_score,
                                int32_t* slot_cat, int32_t* slot_rank, uint64_t* slot_matched, uint64_t* slot_ignored, int32_t* npig,
                                void* stream) {
    STL_CHECK(num_images >= 0 && N >= 0 && N < (1ll << 31) && G >= 0 && G < (1ll << 31), "oks_ap_match: %d images, N = %lld, G = %lld",
              num_images, (long long)N, (long long)G);
    STL_CHECK(max_n >= 0 && max_n <= STL_BOX_MAX, "oks_ap_match: max_n = %d (at most %d detections per image)", max_n, STL_BOX_MAX);
    STL_CHECK(max_g >= 0 && max_g <= STL_BOX_AP_GT_MAX, "oks_ap_match: max_g = %d (at most %d ground truths per image)", max_g,
              STL_BOX_AP_GT_MAX);
    STL_CHECK(oks_thrs && area_ranges && var, "oks_ap_match: null thresholds, area ranges or var");
    if (num_images == 0) return 0;
    STL_CHECK(det_offsets && gt_offsets && npig, "oks_ap_match: null pointer");
    STL_CHECK(N == 0 || (kpts && scores && slot_score && slot_cat && slot_rank && slot_matched && slot_ignored),
              "oks_ap_match: null detection or slot pointer");
    STL_CHECK(G == 0 || (gt_kpts && gt_area && gt_bbox && gt_crowd && gt_numkp), "oks_ap_match: null ground-truth pointer");
    MatchArgs a{};
    a.kpts = kpts, a.scores = scores, a.area = area, a.det_offsets = det_offsets;
    a.gt_kpts = gt_kpts, a.gt_area = gt_area, a.gt_bbox = gt_bbox, a.gt_crowd = gt_crowd, a.gt_numkp = gt_numkp, a.gt_offsets = gt_offsets;
    a.N = N, a.G = G;
    for (int k = 0; k < kJ; ++k) a.var[k] = var[k];
    a.slot_score = slot_score, a.slot_cat = slot_cat, a.slot_rank = slot_rank, a.slot_matched = slot_matched;
    a.slot_ignored = slot_ignored, a.npig = npig;
    // 48 KiB of keys and 20 KiB of OKS at the two caps (71 KiB in all, of the 160 KiB a workgroup can have)
    const auto lds_of = [](const MatchArgs& m) {
        const size_t mg = (size_t)m.max_g;
        return (size_t)m.key_cap * 12 + (size_t)kDets * mg * 8 + mg * 8 + (size_t)kDets * 8 + kA * mg + 2 * mg;
    };
    return launch_match("oks_ap_match", oks_ap_match_kernel, a, oks_thrs, area_ranges, max_n, max_g, num_images, 1, lds_of, ST);
}
