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

namespace {

constexpr int kMatchThreads = 256;
constexpr int kT = STL_BOX_AP_THRS, kA = STL_BOX_AP_AREAS, kChains = kT * kA;   // 40 chains: one lane each, bit t * kA + a
constexpr int kDets = STL_BOX_AP_DETS;
static_assert(kChains <= 64, "one wave runs the chains and one 64-bit word per slot holds their bits");
static_assert(STL_BOX_AP_GT_MAX <= 128, "a chain keeps its matched flags in two 64-bit registers");

// Ascending order of this key = descending score, -0 == +0 (NaN is refused by the wrapper).  With the image-local row in the low
// 32 bits the keys are unique: any sort on them is the stable order of argsort(-score, kind="mergesort").
__device__ __forceinline__ uint64_t score_key(float s, uint32_t row) {
    uint32_t b = s == 0.f ? 0u : __float_as_uint(s);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending with the score
    return ((uint64_t)~b << 32) | row;
}

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

struct MatchArgs {
    const double* boxes;         // [N, 4] xywh
    const float* scores;         // [N]
    const int64_t* labels;       // [N]
    const int64_t* det_offsets;  // [I + 1]
    const double* gt_boxes;      // [G, 4] xywh
    const double* gt_area;       // [G]
    const int64_t* gt_label;     // [G]
    const uint8_t* gt_crowd;     // [G]
    const int64_t* gt_offsets;   // [I + 1]
    const int64_t* cats;         // [K]
    int64_t N, G;
    int K, max_n, key_cap, max_g;
    double thr[kT], lo[kA], hi[kA];
    float* slot_score;           // [N]
    int32_t* slot_cat;           // [N]
    int32_t* slot_rank;          // [N]
    uint64_t* slot_matched;      // [N]
    uint64_t* slot_ignored;      // [N]
    int32_t* npig;               // [I, K, kA]
};

// LDS: skey [key_cap] u64 | siou [kDets * max_g] f64 | sgbox [max_g * 4] f64 | sgarea [max_g] f64 | sdbox [kDets * 4] f64
//      | sgrow [max_g] i32 | sgord [kA * max_g] u8 | sgcrowd [max_g] u8
__global__ __launch_bounds__(kMatchThreads) void box_ap_match_kernel(const MatchArgs a) {
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
    if (o0 < 0 || o1 < o0 || o1 > a.N || o1 - o0 > a.max_n || g0 < 0 || g1 < g0 || g1 > a.G) {   // refused: the wrapper checks first
        if (tid < kA) npig_out[tid] = -1;
        return;
    }
    const int n = (int)(o1 - o0);
    const int64_t cat = a.cats[k];
    if (tid == 0) s_m = 0, s_before = 0, s_g = 0;
    __syncthreads();

    // 1. the image's detections of this category.  The keys are unique, so the order in which they are collected is immaterial.
    //    The category's slots start behind those of every smaller label: the slot ranges of one image never overlap.
    for (int r = tid; r < n; r += kMatchThreads) {
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

    // 3. stable sort by descending score: bitonic over the keys padded to a power of two (padding sorts last)
    int np = 1;
    while (np < m) np <<= 1;
    for (int p = m + tid; p < np; p += kMatchThreads) skey[p] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= np; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (np >> 1); i += kMatchThreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const uint64_t x = skey[lo], y = skey[hi];
                if ((x > y) == ((lo & kk) == 0)) skey[lo] = y, skey[hi] = x;
            }
            __syncthreads();
        }
    }
    const int nd = m < kDets ? m : kDets;

    // 4. stage the kept detections and the ground truth
    for (int e = tid; e < nd * 4; e += kMatchThreads) sdbox[e] = a.boxes[(o0 + (int)(uint32_t)skey[e >> 2]) * 4 + (e & 3)];
    for (int e = tid; e < ng * 4; e += kMatchThreads) sgbox[e] = a.gt_boxes[(g0 + sgrow[e >> 2]) * 4 + (e & 3)];
    for (int g = tid; g < ng; g += kMatchThreads) {
        sgarea[g] = a.gt_area[g0 + sgrow[g]];
        sgcrowd[g] = a.gt_crowd[g0 + sgrow[g]] != 0;
    }
    __syncthreads();

    // 5. per area range: the ground truth with the non-ignored entries first, stable (ignored: crowd, or area outside the range)
    if (tid < kA) {
        const double lo = a.lo[tid], hi = a.hi[tid];
        uint8_t* ord = sgord + tid * mg;
        int c = 0;
        for (int g = 0; g < ng; ++g)
            if (!(sgcrowd[g] || sgarea[g] < lo || sgarea[g] > hi)) ord[c++] = (uint8_t)g;
        s_npig[tid] = c;
        for (int g = 0; g < ng; ++g)
            if (sgcrowd[g] || sgarea[g] < lo || sgarea[g] > hi) ord[c++] = (uint8_t)g;
        npig_out[tid] = s_npig[tid];
    }
    // 6. the IoU tile, fp64
    for (int e = tid; e < nd * ng; e += kMatchThreads) {
        const int d = e / ng, g = e - d * ng;
        siou[e] = bb_iou(sdbox + d * 4, sgbox + g * 4, sgcrowd[g]);
    }
    __syncthreads();
    if (tid >= 64) return;

    // 7. the greedy match: lane c runs the chain of threshold c / kA and area range c % kA over the detections in score order;
    //    its matched flags (by position in that range's order) live in two registers
    const bool chain = lane < kChains;
    const int t = chain ? lane / kA : 0, ar = chain ? lane % kA : 0;
    const double thr0 = a.thr[t] < 1 - 1e-10 ? a.thr[t] : 1 - 1e-10;
    const double lo = a.lo[ar], hi = a.hi[ar];
    const uint8_t* ord = sgord + ar * mg;
    const int nreg = s_npig[ar];          // positions >= nreg are the ignored ones
    const int walk = chain ? ng : 0;
    uint64_t gtm0 = 0, gtm1 = 0;
    const int64_t base = o0 + s_before;
    for (int d = 0; d < nd; ++d) {
        double best = thr0;
        int mt = -1;
        for (int gi = 0; gi < walk; ++gi) {
            const int g = ord[gi];
            if ((((gi < 64 ? gtm0 : gtm1) >> (gi & 63)) & 1) && !sgcrowd[g]) continue;   // already matched, and not a crowd
            if (mt > -1 && mt < nreg && gi >= nreg) break;                                  // matched a regular one: stop at the ignored
            const double v = siou[d * ng + g];
            if (v < best) continue;
            best = v, mt = gi;                                                              // a tie moves to the later ground truth
        }
        bool ign;
        if (mt > -1) {
            ign = mt >= nreg;
            if (mt < 64) gtm0 |= 1ull << mt;
            else gtm1 |= 1ull << (mt - 64);
        } else {
            const double da = sdbox[d * 4 + 2] * sdbox[d * 4 + 3];
            ign = da < lo || da > hi;
        }
        const uint64_t mb = __ballot(chain && mt > -1), ib = __ballot(chain && ign);
        if (lane == 0) {
            const uint64_t key = skey[d];
            const int r = (int)(uint32_t)key;
            a.slot_score[base + d] = a.scores[o0 + r];
            a.slot_cat[base + d] = k;
            a.slot_rank[base + d] = d;
            a.slot_matched[base + d] = mb;
            a.slot_ignored[base + d] = ib;
        }
    }
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
    a.N = N, a.G = G, a.K = K, a.max_n = max_n, a.max_g = max_g > 0 ? max_g : 1;
    a.key_cap = 1;
    while (a.key_cap < (max_n > 0 ? max_n : 1)) a.key_cap <<= 1;
    for (int t = 0; t < kT; ++t) a.thr[t] = iou_thrs[t];
    for (int r = 0; r < kA; ++r) a.lo[r] = area_ranges[2 * r], a.hi[r] = area_ranges[2 * r + 1];
    a.slot_score = slot_score, a.slot_cat = slot_cat, a.slot_rank = slot_rank, a.slot_matched = slot_matched;
    a.slot_ignored = slot_ignored, a.npig = npig;
    const size_t mg = (size_t)a.max_g;
    // 32 KiB of keys and 100 KiB of IoU at the two caps (141 KiB with the staged boxes, of the 160 KiB a workgroup can have); 1 KiB and 13 KiB at 100 detections and 16
    // ground truths per image
    const size_t lds = (size_t)a.key_cap * 8 + (size_t)kDets * mg * 8 + mg * 4 * 8 + mg * 8 + (size_t)kDets * 4 * 8 + mg * 4 + kA * mg + mg;
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&box_ap_match_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    STL_CHECK(ea == hipSuccess, "box_ap_match: %zu bytes of dynamic LDS refused (max_n = %d, max_g = %d): %s", lds, max_n, max_g,
              hipGetErrorString(ea));
    for (int i0 = 0; i0 < num_images; i0 += 1 << 20) {   // grid.x is the image: any number of them
        MatchArgs b = a;
        const int ni = num_images - i0 < (1 << 20) ? num_images - i0 : (1 << 20);
        b.det_offsets += i0, b.gt_offsets += i0, b.npig += (size_t)i0 * K * kA;
        STL_LAUNCH(box_ap_match_kernel, dim3(ni, K), dim3(kMatchThreads), lds, ST, b);
        STL_LAUNCH_CHECK("box_ap_match");
    }
    return 0;
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
