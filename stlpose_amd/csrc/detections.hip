// The detector's device tail on gfx950: head outputs -> final per-image detections -> a ragged store, with no host step between.
//
//   stl_det_postprocess  filter + sort + decode + class-aware greedy NMS + inverse resize, one launch, one workgroup per image.
//   stl_det_append       one launch that appends a batch's rows to a ragged store (xywh fp64, scores, labels, slot table).
//
// Exactness.  The host path this restates is stl_det_decode, torch.sort(stable=True, descending=True), stl_det_nms and
// efficientdet.invert_affine.  fp contract is off for this file (build.py passes -ffp-contract=off as well): the decode, the IoU and
// the two divisions are evaluated as written, in the order detector.hip writes them, so the outputs agree bit for bit.
#include "common.cuh"
#include "../../include/stlpose_hip_detections.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 1024;   // one workgroup per image
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;        // NMS sweep tile: one wave resolves a tile's survivors
constexpr int kMax = STL_BOX_MAX;
constexpr int kPer = kMax / kThreads;   // sorted positions per thread

// as score_key of topdown.hip: ascending key = descending score, NaN first, -0 == +0; the position makes the key unique
__device__ __forceinline__ uint64_t score_key(float s, uint32_t row) {
    uint32_t b = s != s ? 0x7fc00000u : (s == 0.f ? 0u : __float_as_uint(s));
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)~b << 32) | row;
}

// iou_tv of detector.hip: a the kept box, b the later one
__device__ __forceinline__ float iou_tv(const float4 a, const float4 b) {
#pragma clang fp contract(off)
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float xx1 = a.x < b.x ? b.x : a.x;
    const float yy1 = a.y < b.y ? b.y : a.y;
    const float xx2 = b.z < a.z ? b.z : a.z;
    const float yy2 = b.w < a.w ? b.w : a.w;
    const float dw = xx2 - xx1, dh = yy2 - yy1;
    const float w = 0.f < dw ? dw : 0.f;
    const float h = 0.f < dh ? dh : 0.f;
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}

__device__ __forceinline__ int block_scan(int v, int* sw, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sw[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const int s = sw[k];
        base += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();   // sw is free again
    total = tot;
    return base + x - v;
}

struct PostArgs {
    const float* reg;
    const float* cls;
    const float* anchors;
    const StlDetImage* images;   // or null
    int A, nc;
    float thr, xmax, ymax, iou_thr;
    float* boxes;
    float* scores;
    int32_t* labels;
    int32_t* count;
};

// LDS (132 KiB + 136 B): skey [kMax] u64 | sbox [kMax] float4 | sidx [kMax] i32 | scls [kMax] i32 | sdead [kMax] u8 | sw, sm | stile
constexpr size_t kPostLds = (size_t)kMax * (8 + 16 + 4 + 4 + 1) + kWaves * 4 + kWaves * 4 + 8;

__global__ __launch_bounds__(kThreads) void det_postprocess_kernel(const PostArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* skey = reinterpret_cast<uint64_t*>(smem);
    float4* sbox = reinterpret_cast<float4*>(skey + kMax);
    int32_t* sidx = reinterpret_cast<int32_t*>(sbox + kMax);
    int32_t* scls = sidx + kMax;
    uint8_t* sdead = reinterpret_cast<uint8_t*>(scls + kMax);
    int* sw = reinterpret_cast<int*>(sdead + kMax);
    float* sm = reinterpret_cast<float*>(sw + kWaves);
    uint64_t* stile = reinterpret_cast<uint64_t*>(sm + kWaves);

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int A = a.A, nc = a.nc;

    // 1. filter (decode_kernel's test), compacted in anchor order: key, anchor and class per candidate position
    int m = 0;
    for (int a0 = 0; a0 < A; a0 += kThreads) {
        const int an = a0 + tid;
        float best = -INFINITY;
        int bc = 0;
        bool pass = false;
        if (an < A) {
            const float* cp = a.cls + ((int64_t)b * A + an) * nc;
            for (int k = 0; k < nc; ++k) {
                const float v = cp[k];
                if (v > best || k == 0) best = v, bc = k;
            }
            pass = best > a.thr;
        }
        int tot;
        const int pos = m + block_scan(pass ? 1 : 0, sw, tot);
        if (pass && pos < kMax) {
            skey[pos] = score_key(best, (uint32_t)pos);
            sidx[pos] = an;
            scls[pos] = bc;
        }
        m += tot;
    }
    if (m > kMax) {   // refused: nothing is written but the count, which names n
        if (tid == 0) a.count[b] = -m - 1;
        return;
    }
    if (m == 0) {
        if (tid == 0) a.count[b] = 0;
        return;
    }

    // 2. stable sort by descending score: bitonic over the keys padded to a power of two (padding sorts last)
    int np = 1;
    while (np < m) np <<= 1;
    for (int p = m + tid; p < np; p += kThreads) skey[p] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (np >> 1); i += kThreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const uint64_t x = skey[lo], y = skey[hi];
                if ((x > y) == ((lo & k) == 0)) skey[lo] = y, skey[hi] = x;
            }
            __syncthreads();
        }
    }

    // 3. anchor and class into score order (through registers: sidx / scls are permuted in place), the boxes decoded as
    //    decode_kernel does, and the largest coordinate of all candidate boxes
    int ra[kPer], rc[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int p = tid + k * kThreads;
        if (p < m) {
            const int r = (int)(uint32_t)skey[p];
            ra[k] = sidx[r], rc[k] = scls[r];
        }
    }
    __syncthreads();
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int p = tid + k * kThreads;
        if (p >= m) continue;
        sidx[p] = ra[k], scls[p] = rc[k], sdead[p] = 0;
        const float4 an = reinterpret_cast<const float4*>(a.anchors)[ra[k]];
        const float4 r = reinterpret_cast<const float4*>(a.reg)[(int64_t)b * A + ra[k]];
        const float yca = (an.x + an.z) / 2.f, xca = (an.y + an.w) / 2.f;
        const float ha = an.z - an.x, wa = an.w - an.y;
        const float w = expf(r.w) * wa, h = expf(r.z) * ha;
        const float yc = r.x * ha + yca, xc = r.y * wa + xca;
        float x1 = xc - w / 2.f, y1 = yc - h / 2.f, x2 = xc + w / 2.f, y2 = yc + h / 2.f;
        x1 = x1 < 0.f ? 0.f : x1;
        y1 = y1 < 0.f ? 0.f : y1;
        x2 = x2 > a.xmax ? a.xmax : x2;
        y2 = y2 > a.ymax ? a.ymax : y2;
        sbox[p] = make_float4(x1, y1, x2, y2);
        mx = fmaxf(mx, fmaxf(fmaxf(x1, y1), fmaxf(x2, y2)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) sm[tid >> 6] = mx;
    __syncthreads();
    mx = sm[0];
    for (int k = 1; k < kWaves; ++k) mx = fmaxf(mx, sm[k]);
    const float step = mx + 1.f;   // nms_prep_kernel: box + class * (max + 1), in fp32
#define SHIFTED(p_, out_)                                                            \
    {                                                                                \
        const float4 bx_ = sbox[p_];                                                 \
        const float off_ = (float)scls[p_] * step;                                   \
        out_ = make_float4(bx_.x + off_, bx_.y + off_, bx_.z + off_, bx_.w + off_); \
    }

    // 4. greedy sweep in tiles of 64 (box_select_kernel's): wave 0 resolves the tile serially with a wave-uniform alive mask,
    //    then every thread suppresses the later boxes against the tile's survivors
    const float thr = a.iou_thr;
    for (int t0 = 0; t0 < m; t0 += kTile) {
        if (tid < 64) {
            const int p = t0 + lane;
            const bool valid = p < m;
            float4 bl = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) SHIFTED(p, bl);
            uint64_t alive = __ballot(valid && !sdead[valid ? p : 0]);
            for (int k = 0; k < kTile; ++k) {
                if (!((alive >> k) & 1)) continue;   // uniform
                float4 bk;
                SHIFTED(t0 + k, bk);
                const bool sup = lane > k && ((alive >> lane) & 1) && iou_tv(bk, bl) > thr;
                alive &= ~__ballot(sup);
            }
            if (valid && !((alive >> lane) & 1)) sdead[p] = 1;
            if (lane == 0) *stile = alive;
        }
        __syncthreads();
        const uint64_t alive = *stile;
        for (int p = t0 + kTile + tid; p < m; p += kThreads) {
            if (sdead[p]) continue;
            float4 bp;
            SHIFTED(p, bp);
            for (uint64_t s = alive; s; s &= s - 1) {
                float4 bk;
                SHIFTED(t0 + __ffsll((unsigned long long)s) - 1, bk);
                if (iou_tv(bk, bp) > thr) {
                    sdead[p] = 1;
                    break;
                }
            }
        }
        __syncthreads();
    }
#undef SHIFTED

    // 5. the survivors in score order, on the source image's scale when the record table is given
    float rx = 1.f, ry = 1.f;
    if (a.images) {
        const StlDetImage im = a.images[b];
        rx = (float)((double)im.new_w / (double)im.old_w);
        ry = (float)((double)im.new_h / (double)im.old_h);
    }
    const int per = (m + kThreads - 1) / kThreads;
    const int q0 = min(m, tid * per), q1 = min(m, q0 + per);
    int alive_n = 0;
    for (int p = q0; p < q1; ++p) alive_n += !sdead[p];
    int kept;
    int out = block_scan(alive_n, sw, kept);
    for (int p = q0; p < q1; ++p) {
        if (sdead[p]) continue;
        float4 bx = sbox[p];
        if (a.images) bx = make_float4(bx.x / rx, bx.y / ry, bx.z / rx, bx.w / ry);
        const int64_t o = (int64_t)b * kMax + out++;
        reinterpret_cast<float4*>(a.boxes)[o] = bx;
        a.scores[o] = a.cls[((int64_t)b * A + sidx[p]) * nc + scls[p]];
        a.labels[o] = scls[p] + 1;
    }
    if (tid == 0) a.count[b] = kept;
}

struct AppendArgs {
    const float* boxes;
    const float* scores;
    const int32_t* labels;
    const int32_t* count;
    const int64_t* image_ids;
    int B;
    double* st_boxes;
    float* st_scores;
    int64_t* st_labels;
    int64_t cap;
    int64_t* slots;
    int64_t slot0;
    int64_t* cursor;
    int parity;
    int64_t* overflow;
};

// grid B, 1024 threads: every workgroup sums the counts before its image (thread i holds image i), then copies its rows.
// cursor[parity] is only read and cursor[1 - parity] only written (by workgroup 0), so the workgroups need no order.
__global__ __launch_bounds__(kThreads) void det_append_kernel(const AppendArgs a) {
#pragma clang fp contract(off)
    __shared__ int sw[kWaves];
    __shared__ int sstart;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int c = tid < a.B ? a.count[tid] : 0;
    int total;
    const int before = block_scan(min(max(c, 0), kMax), sw, total);   // a table holds at most kMax rows per image
    if (tid == b) sstart = before;
    __syncthreads();
    const int64_t base = a.cursor[a.parity];
    const int64_t start = base + sstart;
    const int raw = a.count[b], n = min(raw, kMax);
    if (tid == 0) {
        int64_t* s = a.slots + (a.slot0 + b) * 3;
        s[0] = a.image_ids[b], s[1] = start, s[2] = raw;
        if (b == 0) a.cursor[1 - a.parity] = base + total;
    }
    bool dropped = false;
    for (int k = tid; k < n; k += kThreads) {
        const int64_t row = start + k;
        if (row >= a.cap) {
            dropped = true;
            continue;
        }
        const int64_t o = (int64_t)b * kMax + k;
        const float4 bx = reinterpret_cast<const float4*>(a.boxes)[o];
        const float w = bx.z - bx.x, h = bx.w - bx.y;   // convert_to_xywh in the tensor's own dtype, widened afterwards
        double* d = a.st_boxes + row * 4;
        d[0] = (double)bx.x, d[1] = (double)bx.y, d[2] = (double)w, d[3] = (double)h;
        a.st_scores[row] = a.scores[o];
        a.st_labels[row] = (int64_t)a.labels[o];
    }
    if (dropped) *a.overflow = 1;
}

struct PersonArgs {
    const float* boxes;      // the Detections tables [B, kMax, ...]
    const float* scores;
    const int32_t* labels;
    const int32_t* count;
    int B, label;
    float thr, ar, wo, ho;
    // compacted rows [B * kMax, ...]
    int32_t* img;
    float* rbox;
    float* rscore;
    float* center;
    float* scale;
    float* minv;
    int64_t* offsets;        // [B + 1]
    int32_t* total;
};

// TransformDetection.coords2cs in fp32 as it is written, and the crop -> image matrix of get_affine_transform(rot = 0, inv = 1) in
// closed form: a pure scaling by box width / crop width that takes the crop's centre to the box centre.
__device__ __forceinline__ void person_row(const PersonArgs& a, int64_t o, int image, const float4 bx, float score) {
#pragma clang fp contract(off)
    const float w = bx.z - bx.x, h = bx.w - bx.y;
    const float cx = bx.x + w * 0.5f, cy = bx.y + h * 0.5f;
    const bool wider = w > a.ar * h, taller = w < a.ar * h;
    const float h2 = wider ? w * 1.0f / a.ar : h;
    const float w2 = (!wider && taller) ? h * a.ar : w;
    float sx = w2 * 1.0f / 200.f, sy = h2 * 1.0f / 200.f;
    if (cx != -1.f) sx = sx * 1.25f, sy = sy * 1.25f;
    const float bw = sx * 200.f;   // the reference rounds scale * 200 to fp32 (lib/transforms.py:206)
    const float r = bw / a.wo;
    a.img[o] = image;
    reinterpret_cast<float4*>(a.rbox)[o] = bx;
    a.rscore[o] = score;
    a.center[2 * o] = cx, a.center[2 * o + 1] = cy;
    a.scale[2 * o] = sx, a.scale[2 * o + 1] = sy;
    float* m = a.minv + 6 * o;
    m[0] = r, m[1] = 0.f, m[2] = cx - 0.5f * bw;
    m[3] = 0.f, m[4] = r, m[5] = cy - (0.5f * a.ho) * r;
}

__device__ __forceinline__ bool person_pass(const PersonArgs& a, int64_t o) { return a.labels[o] == a.label && a.scores[o] > a.thr; }

// grid B, 1024 threads: bbox_filtering (label == label and score > thr, in row order) on the tables.  Workgroup b counts the
// passing rows of the images before it for its first row, so the rows of all images are adjacent and in image order.
__global__ __launch_bounds__(kThreads) void person_filter_kernel(const PersonArgs a) {
    __shared__ int sw[kWaves];
    __shared__ int sfirst, sbad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) sfirst = 0, sbad = a.B;
    __syncthreads();
    int mine = 0;
    for (int i = 0; i < b; ++i) {
        const int n = min(a.count[i], kMax);
        if (a.count[i] < 0 && tid == 0) atomicMin(&sbad, i);
        for (int r = tid; r < n; r += kThreads) mine += person_pass(a, (int64_t)i * kMax + r);
    }
    if (mine) atomicAdd(&sfirst, mine);
    __syncthreads();
    const int first = sfirst;
    const int n = min(a.count[b], kMax);   // negative: no rows
    if (a.count[b] < 0 && tid == 0) atomicMin(&sbad, b);
    int done = 0;
    for (int r0 = 0; r0 < n; r0 += kThreads) {
        const int r = r0 + tid;
        const int64_t o = (int64_t)b * kMax + r;
        const bool ok = r < n && person_pass(a, o);
        int tot;
        const int pos = first + done + block_scan(ok ? 1 : 0, sw, tot);
        if (ok) person_row(a, pos, b, reinterpret_cast<const float4*>(a.boxes)[o], a.scores[o]);
        done += tot;
    }
    __syncthreads();
    if (tid == 0) {
        if (b == 0) a.offsets[0] = 0;
        a.offsets[b + 1] = first + done;
        if (b == a.B - 1) *a.total = sbad < a.B ? -sbad - 1 : first + done;   // an image above the cap: -(its index) - 1
    }
}

struct GatherArgs {
    PersonArgs from;             // the filtered rows (img .. minv, offsets)
    const int32_t* keep;         // stl_box_select's: per image segment the kept image-local rows, then -1
    const int32_t* kept;         // [B]
    int32_t* img;
    float* rbox;
    float* rscore;
    float* center;
    float* scale;
    float* minv;
    int32_t* total;
};

// grid B, 1024 threads: the rows stl_box_select kept, in its order, adjacent over the images
__global__ __launch_bounds__(kThreads) void person_gather_kernel(const GatherArgs g) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int first = 0;
    for (int i = 0; i < b; ++i) first += max(g.kept[i], 0);
    const int n = min(max(g.kept[b], 0), kMax);
    const int64_t o0 = g.from.offsets[b];
    for (int k = tid; k < n; k += kThreads) {
        const int64_t s = o0 + g.keep[o0 + k], d = first + k;
        g.img[d] = g.from.img[s];
        reinterpret_cast<float4*>(g.rbox)[d] = reinterpret_cast<const float4*>(g.from.rbox)[s];
        g.rscore[d] = g.from.rscore[s];
        for (int e = 0; e < 2; ++e) g.center[2 * d + e] = g.from.center[2 * s + e], g.scale[2 * d + e] = g.from.scale[2 * s + e];
        for (int e = 0; e < 6; ++e) g.minv[6 * d + e] = g.from.minv[6 * s + e];
    }
    if (tid == 0 && b == g.from.B - 1) *g.total = *g.from.total < 0 ? *g.from.total : first + n;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_det_postprocess(const float* reg, const float* cls, const float* anchors, const void* images, int B, int A, int nc,
                                   float thr, float xmax, float ymax, double iou_thr, float* boxes, float* scores, int32_t* labels,
                                   int32_t* count, void* stream) {
    STL_CHECK(B >= 0 && A >= 0 && nc >= 1, "det_postprocess: B %d A %d nc %d", B, A, nc);
    if (B == 0) return 0;
    STL_CHECK(count && boxes && scores && labels, "det_postprocess: null output");
    STL_CHECK(A == 0 || (reg && cls && anchors), "det_postprocess: null pointer");
    // stl_det_nms's threshold: iou > t (double)  <=>  iou > (the largest float <= t)
    float t = (float)iou_thr;
    if ((double)t > iou_thr) t = nextafterf(t, -INFINITY);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&det_postprocess_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)kPostLds);
    const PostArgs a{reg, cls, anchors, static_cast<const StlDetImage*>(images), A, nc, thr, xmax, ymax, t, boxes, scores, labels, count};
    STL_LAUNCH(det_postprocess_kernel, dim3(B), dim3(kThreads), kPostLds, ST, a);
    STL_LAUNCH_CHECK("det_postprocess");
    return 0;
}

extern "C" int stl_det_append(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count,
                              const int64_t* image_ids, int B, double* st_boxes, float* st_scores, int64_t* st_labels, int64_t cap,
                              int64_t* slots, int64_t slot0, int64_t* cursor, int parity, int64_t* overflow, void* stream) {
    STL_CHECK(B >= 0 && B <= kThreads, "det_append: %d images (at most %d per launch)", B, kThreads);
    STL_CHECK(cap >= 0 && slot0 >= 0 && (parity == 0 || parity == 1), "det_append: cap %lld slot0 %lld parity %d", (long long)cap,
              (long long)slot0, parity);
    if (B == 0) return 0;
    STL_CHECK(boxes && scores && labels && count && image_ids && slots && cursor && overflow, "det_append: null pointer");
    STL_CHECK(cap == 0 || (st_boxes && st_scores && st_labels), "det_append: null store");
    const AppendArgs a{boxes, scores, labels, count, image_ids, B, st_boxes, st_scores, st_labels, cap, slots, slot0, cursor, parity,
                       overflow};
    STL_LAUNCH(det_append_kernel, dim3(B), dim3(kThreads), 0, ST, a);
    STL_LAUNCH_CHECK("det_append");
    return 0;
}

extern "C" int stl_person_boxes(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, int B, int label,
                                float score_thr, double iou_thr, float aspect, int crop_w, int crop_h, void* work, int32_t* img,
                                float* out_boxes, float* out_scores, float* center, float* scale, float* minv, int32_t* total,
                                void* stream) {
    STL_CHECK(B >= 0 && B <= kThreads && crop_w >= 1 && crop_h >= 1 && aspect > 0.f, "person_boxes: B %d, crop %d x %d, aspect %g", B,
              crop_w, crop_h, (double)aspect);
    STL_CHECK(total, "person_boxes: null total");
    if (B == 0) {
        (void)hipMemsetAsync(total, 0, 4, ST);
        return 0;
    }
    STL_CHECK(boxes && scores && labels && count && work && img && out_boxes && out_scores && center && scale && minv,
              "person_boxes: null pointer");
    const bool nms = iou_thr >= 0.0;
    const int64_t N = (int64_t)B * kMax;
    // work: offsets int64 [B + 1] (padded to 16 B) | with NMS also: the filtered rows, keep int32 [N], kept int32 [B], total
    char* w = static_cast<char*>(work);
    int64_t* offsets = reinterpret_cast<int64_t*>(w);
    w += ((int64_t)(B + 1) * 8 + 15) & ~(int64_t)15;
    PersonArgs a{boxes, scores, labels, count, B, label, score_thr, aspect, (float)crop_w, (float)crop_h,
                 img, out_boxes, out_scores, center, scale, minv, offsets, total};
    if (nms) {
        a.rbox = reinterpret_cast<float*>(w), w += N * 16;
        a.minv = reinterpret_cast<float*>(w), w += N * 24;
        a.center = reinterpret_cast<float*>(w), w += N * 8;
        a.scale = reinterpret_cast<float*>(w), w += N * 8;
        a.rscore = reinterpret_cast<float*>(w), w += N * 4;
        a.img = reinterpret_cast<int32_t*>(w), w += N * 4;
    }
    int32_t* keep = reinterpret_cast<int32_t*>(w);
    int32_t* kept = keep + N;
    if (nms) a.total = kept + B;
    STL_LAUNCH(person_filter_kernel, dim3(B), dim3(kThreads), 0, ST, a);
    STL_LAUNCH_CHECK("person_filter");
    if (!nms) return 0;
    // torchvision.ops.nms on the passing rows, as bbox_nms calls it: no label or score test left, N rows promised at most
    if (int rc = stl_box_select(a.rbox, a.rscore, nullptr, offsets, B, N, kMax, 0, 0, 0.f, iou_thr, keep, kept, stream)) return rc;
    const GatherArgs g{a, keep, kept, img, out_boxes, out_scores, center, scale, minv, total};
    STL_LAUNCH(person_gather_kernel, dim3(B), dim3(kThreads), 0, ST, g);
    STL_LAUNCH_CHECK("person_gather");
    return 0;
}

extern "C" int64_t stl_person_boxes_workspace(int B, int nms) {
    const int64_t N = (int64_t)B * kMax;
    return (((int64_t)(B + 1) * 8 + 15) & ~(int64_t)15) + (nms ? N * (16 + 24 + 8 + 8 + 4 + 4) + N * 4 + (int64_t)B * 4 + 16 : 0);
}
