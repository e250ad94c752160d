// COCO box AP on gfx950: the detector's validation metric (02_train_faster_rcnn.py:241-280, 03_evaluate_faster_rcnn.py:119-184 score
// with pycocotools' COCOeval(..., "bbox"); this file restates the published algorithm of that class).
//
//   stl_box_ap_match       COCOeval.evaluateImg for iouType "bbox": one workgroup per (image, category) sorts the image's detections of
//                          that category (stable, descending score, the first STL_BOX_AP_DETS kept), computes their IoU with the
//                          category's ground truth as maskApi.bbIou does and runs the greedy match for every (threshold, area range).
//   stl_box_ap_accumulate  COCOeval.accumulate and the reductions summarize needs: one workgroup per (threshold, area range, maxDets,
//                          category) scans the category's slots in global score order.  It reads match / ignore bits, ranks and
//                          counts only: nothing in it knows what was matched.
//
// Exactness.  fp contract is off for this file: dw * dh + gw * gh - w * h must not become an FMA, or an IoU that sits exactly on a
// threshold flips.  IoU, recall (tp / npig) and precision (tp / (fp + tp + 2^-52)) are each evaluated in fp64 exactly as written
// here; every sum is an integer and every maximum is order-free.  The result is therefore deterministic and equals an fp64 numpy
// restatement (tests/box_ap_ref.py) bit for bit.
#include "common.cuh"

#pragma clang fp contract(off)

#include "coco_match.inc"

namespace {

constexpr int kT = STL_BOX_AP_THRS, kA = STL_BOX_AP_AREAS;   // 40 chains
constexpr int kDets = STL_BOX_AP_DETS;

// Ascending order of this key = descending score (NaN is refused by the wrapper).  With the image-local row in the low 32 bits the
// keys are unique: any sort on them is the stable order of argsort(-score, kind="mergesort").
__device__ __forceinline__ uint64_t score_key(float s, uint32_t row) { return ((uint64_t)(uint32_t)~score_bits(s) << 32) | row; }

// maskApi.bbIou for one (detection, ground truth) pair, boxes as (x, y, w, h).
__device__ __forceinline__ double bb_iou(const double* d, const double* g, bool crowd) {
#pragma clang fp contract(off)
    const double ga = g[2] * g[3], da = d[2] * d[3];
    const double xr = d[2] + d[0], gxr = g[2] + g[0];
    const double w = (xr < gxr ? xr : gxr) - (d[0] > g[0] ? d[0] : g[0]);
    if (w <= 0) return 0.0;
    const double yb = d[3] + d[1], gyb = g[3] + g[1];
    const double h = (yb < gyb ? yb : gyb) - (d[1] > g[1] ? d[1] : g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

struct MatchArgs : MatchBase<kT, kA, float> {
    const double* boxes;         // [N, 4] xywh
    const int64_t* labels;       // [N]
    const double* gt_boxes;      // [G, 4] xywh
    const double* gt_area;       // [G]
    const int64_t* gt_label;     // [G]
    const uint8_t* gt_crowd;     // [G]
    const int64_t* cats;         // [K]
};

// LDS: skey [key_cap] u64 | siou [kDets * max_g] f64 | sgbox [max_g * 4] f64 | sgarea [max_g] f64 | sdbox [kDets * 4] f64
//      | sgrow [max_g] i32 | sgord [kA * max_g] u8 | sgcrowd [max_g] u8
__global__ __launch_bounds__(kThreads) void box_ap_match_kernel(const MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int mg = a.max_g;
    uint64_t* skey = reinterpret_cast<uint64_t*>(smem);
    double* siou = reinterpret_cast<double*>(skey + a.key_cap);
    double* sgbox = siou + (size_t)kDets * mg;
    double* sgarea = sgbox + (size_t)mg * 4;
    double* sdbox = sgarea + mg;
    int32_t* sgrow = reinterpret_cast<int32_t*>(sdbox + kDets * 4);
    uint8_t* sgord = reinterpret_cast<uint8_t*>(sgrow + mg);
    uint8_t* sgcrowd = sgord + kA * mg;
    __shared__ int s_m, s_before, s_g, s_npig[kA];

    const int img = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    int32_t* npig_out = a.npig + ((size_t)img * a.K + k) * kA;
    const int64_t o0 = a.det_offsets[img], o1 = a.det_offsets[img + 1];
    const int64_t g0 = a.gt_offsets[img], g1 = a.gt_offsets[img + 1];
    if (offsets_refused(a, o0, o1, g0, g1)) {   // the wrapper checks first
        if (tid < kA) npig_out[tid] = -1;
        return;
    }
    const int n = (int)(o1 - o0);
    const int64_t cat = a.cats[k];
    if (tid == 0) s_m = 0, s_before = 0, s_g = 0;
    __syncthreads();

    // 1. the image's detections of this category.  The keys are unique, so the order in which they are collected is immaterial.
    //    The category's slots start behind those of every smaller label: the slot ranges of one image never overlap.
    for (int r = tid; r < n; r += kThreads) {
        const int64_t l = a.labels[o0 + r];
        if (l == cat) skey[atomicAdd(&s_m, 1)] = score_key(a.scores[o0 + r], (uint32_t)r);
        else if (l < cat) atomicAdd(&s_before, 1);
    }
    // 2. its ground truth of this category, in input order (wave 0, 64 rows at a time)
    if (tid < 64) {
        int cnt = 0;
        for (int64_t r0 = g0; r0 < g1; r0 += 64) {
            const int64_t r = r0 + lane;
            const bool is = r < g1 && a.gt_label[r] == cat;
            const uint64_t mask = __ballot(is);
            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1));
            if (is && pos < mg) sgrow[pos] = (int32_t)(r - g0);
            cnt += __popcll(mask);
        }
        if (lane == 0) s_g = cnt;
    }
    __syncthreads();
    const int m = s_m, ng = s_g;
    if (ng > mg) {   // above the cap the wrapper checked: refused
        if (tid < kA) npig_out[tid] = -1;
        return;
    }

    // 3. stable sort by descending score
    bitonic_sort<false>(skey, nullptr, m, tid);
    const int nd = m < kDets ? m : kDets;

    // 4. stage the kept detections and the ground truth
    for (int e = tid; e < nd * 4; e += kThreads) sdbox[e] = a.boxes[(o0 + (int)(uint32_t)skey[e >> 2]) * 4 + (e & 3)];
    for (int e = tid; e < ng * 4; e += kThreads) sgbox[e] = a.gt_boxes[(g0 + sgrow[e >> 2]) * 4 + (e & 3)];
    for (int g = tid; g < ng; g += kThreads) {
        sgarea[g] = a.gt_area[g0 + sgrow[g]];
        sgcrowd[g] = a.gt_crowd[g0 + sgrow[g]] != 0;
    }
    __syncthreads();

    // 5. the ground truth in each area range's order (ignored: a crowd, or outside the range)
    order_ground_truth(a, sgcrowd, sgarea, ng, sgord, s_npig, npig_out, tid);
    // 6. the IoU tile, fp64
    for (int e = tid; e < nd * ng; e += kThreads) {
        const int d = e / ng, g = e - d * ng;
        siou[e] = bb_iou(sdbox + d * 4, sgbox + g * 4, sgcrowd[g]);
    }
    __syncthreads();
    if (tid >= 64) return;

    // 7. the greedy match
    greedy_match(a, siou, sgcrowd, sgord, s_npig, nd, ng, o0, o0 + s_before, k,
                 [&](int d) { return sdbox[d * 4 + 2] * sdbox[d * 4 + 3]; }, [&](int d) { return (int)(uint32_t)skey[d]; }, lane);
}

constexpr int kAccThreads = STL_BOX_AP_SCAN_TILE;   // one slot per thread and tile
constexpr int kAccWaves = kAccThreads / 64;

struct AccArgs {
    const uint64_t* matched;      // [S]
    const uint64_t* ignored;      // [S]
    const int32_t* rank;          // [S]
    const int64_t* order;         // [S]
    const int64_t* cat_offsets;   // [K + 1]
    const int64_t* npig;          // [K, A]
    int64_t S;
    int K, T, A, M, R;
    int max_dets[STL_BOX_AP_MAXDETS_MAX];
    double rec[STL_BOX_AP_RECS_MAX];
    double* precision;            // [T, R, K, A, M]
    double* recall;               // [T, K, A, M]
};

__global__ __launch_bounds__(kAccThreads) void box_ap_accumulate_kernel(const AccArgs a) {
    __shared__ double srec[STL_BOX_AP_RECS_MAX];
    __shared__ unsigned long long sbin[STL_BOX_AP_RECS_MAX];
    __shared__ int swt[kAccWaves], swf[kAccWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = blockIdx.y;
    const int mi = blockIdx.x % a.M, ai = (blockIdx.x / a.M) % a.A, ti = blockIdx.x / (a.M * a.A);
    const int bit = ti * a.A + ai, R = a.R;
    double* prec = a.precision + (((size_t)ti * R * a.K + k) * a.A + ai) * a.M + mi;   // + r * K * A * M
    const size_t rstride = (size_t)a.K * a.A * a.M;
    double* rec_out = a.recall + (((size_t)ti * a.K + k) * a.A + ai) * a.M + mi;
    const int64_t npig = a.npig[(size_t)k * a.A + ai];
    const int64_t s0 = a.cat_offsets[k], s1 = a.cat_offsets[k + 1];
    if (npig <= 0 || s0 < 0 || s1 < s0 || s1 > a.S) {   // no ground truth to find: the entries stay -1
        for (int r = tid; r < R; r += kAccThreads) prec[r * rstride] = -1.0;
        if (tid == 0) *rec_out = -1.0;
        return;
    }
    for (int r = tid; r < R; r += kAccThreads) srec[r] = a.rec[r], sbin[r] = 0ull;
    __syncthreads();
    const int maxdet = a.max_dets[mi];
    const double dn = (double)npig;
    int ctp = 0, cfp = 0;   // true / false positives of the tiles before this one
    for (int64_t p0 = s0; p0 < s1; p0 += kAccThreads) {
        const int64_t p = p0 + tid;
        int tp = 0, fp = 0;
        if (p < s1) {
            const int64_t o = a.order[p];
            if (o >= 0 && o < a.S && a.rank[o] < maxdet) {
                const int mb = (int)((a.matched[o] >> bit) & 1), ib = (int)((a.ignored[o] >> bit) & 1);
                tp = mb & (ib ^ 1), fp = (mb ^ 1) & (ib ^ 1);
            }
        }
        // inclusive scan of both counts: wave-64 shuffles, then the wave totals through LDS
        int xt = tp, xf = fp;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int yt = __shfl_up(xt, o), yf = __shfl_up(xf, o);
            if (lane >= o) xt += yt, xf += yf;
        }
        if (lane == 63) swt[wv] = xt, swf[wv] = xf;
        __syncthreads();
        int bt = 0, bf = 0, tt = 0, tf = 0;
#pragma unroll
        for (int w = 0; w < kAccWaves; ++w) {
            const int st = swt[w], sf = swf[w];
            bt += w < wv ? st : 0, bf += w < wv ? sf : 0;
            tt += st, tf += sf;
        }
        __syncthreads();   // swt / swf are free again
        if (tp) {
            const int tpi = ctp + bt + xt, fpi = cfp + bf + xf;
            const double rc = (double)tpi / dn;
            const double pr = (double)tpi / (((double)fpi + (double)tpi) + 0x1p-52);
            int lo = 0, hi = R;   // the last recall point <= rc (rc > 0 = rec[0]: there is one)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (srec[mid] <= rc) lo = mid;
                else hi = mid;
            }
            atomicMax(&sbin[lo], (unsigned long long)__double_as_longlong(pr));   // pr > 0: its bits order as an integer
        }
        ctp += tt, cfp += tf;
    }
    __syncthreads();
    // precision at recall point r = the largest bin maximum at or behind it; bins nothing reached give 0
    if (tid < 64) {
        unsigned long long run = 0ull;   // the suffix maximum of the chunks behind this one
        for (int c0 = ((R - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
            const int r = c0 + lane;
            unsigned long long x = r < R ? sbin[r] : 0ull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long y = __shfl_down(x, o);
                if (lane + o < 64 && y > x) x = y;
            }
            if (run > x) x = run;
            if (r < R) prec[r * rstride] = __longlong_as_double((long long)x);
            run = __shfl(x, 0);
        }
    }
    if (tid == 0) *rec_out = (double)ctp / dn;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_box_ap_match(const double* boxes, const float* scores, const int64_t* labels, const int64_t* det_offsets, int64_t N,
                                int max_n, const double* gt_boxes, const double* gt_area, const int64_t* gt_label,
                                const uint8_t* gt_crowd, const int64_t* gt_offsets, int64_t G, int max_g, int num_images,
                                const int64_t* cats, int K, const double* iou_thrs, const double* area_ranges, float* slot_score,
                                int32_t* slot_cat, int32_t* slot_rank, uint64_t* slot_matched, uint64_t* slot_ignored, int32_t* npig,
                                void* stream) {
    STL_CHECK(num_images >= 0 && K >= 0 && K <= 65535 && N >= 0 && N < (1ll << 31) && G >= 0 && G < (1ll << 31),
              "box_ap_match: %d images, %d categories, N = %lld, G = %lld", num_images, K, (long long)N, (long long)G);
    STL_CHECK(max_n >= 0 && max_n <= STL_BOX_MAX, "box_ap_match: max_n = %d (at most %d detections per image)", max_n, STL_BOX_MAX);
    STL_CHECK(max_g >= 0 && max_g <= STL_BOX_AP_GT_MAX, "box_ap_match: max_g = %d (at most %d ground truths per image and category)",
              max_g, STL_BOX_AP_GT_MAX);
    STL_CHECK(iou_thrs && area_ranges, "box_ap_match: null thresholds or area ranges");
    if (num_images == 0 || K == 0) return 0;
    STL_CHECK(det_offsets && gt_offsets && cats && npig, "box_ap_match: null pointer");
    STL_CHECK(N == 0 || (boxes && scores && labels && slot_score && slot_cat && slot_rank && slot_matched && slot_ignored),
              "box_ap_match: null detection or slot pointer");
    STL_CHECK(G == 0 || (gt_boxes && gt_area && gt_label && gt_crowd), "box_ap_match: null ground-truth pointer");
    MatchArgs a{};
    a.boxes = boxes, a.scores = scores, a.labels = labels, a.det_offsets = det_offsets;
    a.gt_boxes = gt_boxes, a.gt_area = gt_area, a.gt_label = gt_label, a.gt_crowd = gt_crowd, a.gt_offsets = gt_offsets, a.cats = cats;
    a.N = N, a.G = G;
    a.slot_score = slot_score, a.slot_cat = slot_cat, a.slot_rank = slot_rank, a.slot_matched = slot_matched;
    a.slot_ignored = slot_ignored, a.npig = npig;
    // 32 KiB of keys and 100 KiB of IoU at the two caps (141 KiB with the staged boxes, of the 160 KiB a workgroup can have); 1 KiB and 13 KiB at 100 detections and 16
    // ground truths per image
    const auto lds_of = [](const MatchArgs& m) {
        const size_t mg = (size_t)m.max_g;
        return (size_t)m.key_cap * 8 + (size_t)kDets * mg * 8 + mg * 4 * 8 + mg * 8 + (size_t)kDets * 4 * 8 + mg * 4 + kA * mg + mg;
    };
    return launch_match("box_ap_match", box_ap_match_kernel, a, iou_thrs, area_ranges, max_n, max_g, num_images, K, lds_of, ST);
}

extern "C" int stl_box_ap_accumulate(const uint64_t* matched, const uint64_t* ignored, const int32_t* rank, const int64_t* order,
                                     const int64_t* cat_offsets, const int64_t* npig, int64_t S, int K, int T, int A,
                                     const int32_t* max_dets, int M, const double* rec_thrs, int R, double* precision, double* recall,
                                     void* stream) {
    STL_CHECK(S >= 0 && S < (1ll << 31) && K >= 0 && K <= 65535, "box_ap_accumulate: S = %lld slots, %d categories", (long long)S, K);
    STL_CHECK(T >= 1 && A >= 1 && T * A <= 64, "box_ap_accumulate: T = %d, A = %d (T * A <= 64 bits per slot)", T, A);
    STL_CHECK(M >= 1 && M <= STL_BOX_AP_MAXDETS_MAX && max_dets, "box_ap_accumulate: %d maxDets (1 .. %d)", M, STL_BOX_AP_MAXDETS_MAX);
    STL_CHECK(R >= 1 && R <= STL_BOX_AP_RECS_MAX && rec_thrs, "box_ap_accumulate: %d recall points (1 .. %d)", R, STL_BOX_AP_RECS_MAX);
    STL_CHECK(rec_thrs[0] == 0.0, "box_ap_accumulate: the first recall point must be 0");
    for (int r = 1; r < R; ++r) STL_CHECK(rec_thrs[r] > rec_thrs[r - 1], "box_ap_accumulate: the recall points must rise");
    STL_CHECK((int64_t)T * A * M < (1ll << 31), "box_ap_accumulate: grid");
    if (K == 0) return 0;
    STL_CHECK(cat_offsets && npig && precision && recall, "box_ap_accumulate: null pointer");
    STL_CHECK(S == 0 || (matched && ignored && rank && order), "box_ap_accumulate: null slot pointer");
    AccArgs a{};
    a.matched = matched, a.ignored = ignored, a.rank = rank, a.order = order, a.cat_offsets = cat_offsets, a.npig = npig;
    a.S = S, a.K = K, a.T = T, a.A = A, a.M = M, a.R = R;
    for (int m = 0; m < M; ++m) a.max_dets[m] = max_dets[m];
    for (int r = 0; r < R; ++r) a.rec[r] = rec_thrs[r];
    a.precision = precision, a.recall = recall;
    STL_LAUNCH(box_ap_accumulate_kernel, dim3(T * A * M, K), dim3(kAccThreads), 0, ST, a);
    STL_LAUNCH_CHECK("box_ap_accumulate");
    return 0;
}
