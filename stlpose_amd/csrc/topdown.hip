// Top-down pose extraction on gfx950: the glue between a person detector and HRNet (04_evaluate_vases_qualitatively.py:184-250,
// 05_create_archdata_retrieval_db.py:114-171).
//
//   stl_box_select             per-image label / score filter (lib/bounding_box.py:127-168) and greedy NMS with the semantics of
//                              torchvision.ops.nms as bbox_nms (:171-206) calls it, for a ragged batch of images in one launch.
//   stl_heatmap_resize_argmax  F.interpolate(..., (Ho, Wo), bilinear, align_corners=True) fused with get_max_preds_hrnet
//                              (lib/pose_parsing.py:16-55): the upsampled maps are computed in registers, never written.
//
// Exactness.  fp contract is off for this file: the IoU and the interpolation are evaluated exactly as written, so a float32
// restatement with the same operation order (tests/topdown_ref.py) reproduces them bit for bit.
#include "common.cuh"

#pragma clang fp contract(off)

namespace {

constexpr int kBoxThreads = 1024;   // one workgroup per image
constexpr int kBoxWaves = kBoxThreads / 64;
constexpr int kTile = 64;           // NMS sweep tile: one wave resolves a tile's survivors

// Ascending order of this key = descending score, every NaN first (torch.sort(descending=True) puts NaN ahead of +inf),
// -0 == +0.  With the row index in the low 32 bits the keys are unique: any sort on them is stable by construction.
__device__ __forceinline__ uint64_t score_key(float s, uint32_t row) {
    uint32_t b = s != s ? 0x7fc00000u : (s == 0.f ? 0u : __float_as_uint(s));
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending with the score
    return ((uint64_t)~b << 32) | row;
}

// IoU of the kept box a with the candidate b, as torchvision's nms_kernel computes it (x1, y1, x2, y2; no +1):
// std::max / std::min written out, inter / (area_a + area_b - inter) left to right, nothing contracted.
__device__ __forceinline__ float box_iou(const float4 a, const float4 b) {
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

// Exclusive prefix sum of v over the workgroup (kBoxThreads threads); total: the sum.  sw: kBoxWaves ints of LDS.
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
    for (int k = 0; k < kBoxWaves; ++k) {
        const int s = sw[k];
        base += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();   // sw is free again
    total = tot;
    return base + x - v;
}

struct BoxArgs {
    const float* boxes;      // [N, 4]
    const float* scores;     // [N]
    const int64_t* labels;   // [N] or null: no label test
    const int64_t* offsets;  // [I + 1]
    int64_t N, label;
    float score_thr, iou_thr;
    int32_t* keep;           // [N]
    int32_t* count;          // [I]
    int max_n, key_cap, nms, score_test;   // key_cap: max_n rounded up to a power of two
};

// LDS: skey [key_cap] u64 | sbox [max_n] float4 | sdead [max_n] u8 | sw [16] int | stile u64
__global__ __launch_bounds__(kBoxThreads) void box_select_kernel(const BoxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* skey = reinterpret_cast<uint64_t*>(smem);
    float4* sbox = reinterpret_cast<float4*>(skey + a.key_cap);
    uint8_t* sdead = reinterpret_cast<uint8_t*>(sbox + a.max_n);
    int* sw = reinterpret_cast<int*>(sdead + ((a.max_n + 15) & ~15));
    uint64_t* stile = reinterpret_cast<uint64_t*>(sw + kBoxWaves);

    const int img = blockIdx.x, tid = threadIdx.x;
    const int64_t o0 = a.offsets[img], o1 = a.offsets[img + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.N || o1 - o0 > a.max_n) {   // refused (the wrapper checks first): nothing is touched
        if (tid == 0) a.count[img] = -1;
        return;
    }
    const int n = (int)(o1 - o0);
    int32_t* keep = a.keep + o0;

    // 1. filter (bounding_box.py:152): rows [tid * per, tid * per + per) per thread, compacted in row order
    const int per = (n + kBoxThreads - 1) / kBoxThreads;   // <= 4
    const int r0 = tid * per;
    int pass = 0;
    for (int r = r0; r < r0 + per && r < n; ++r) {
        const float s = a.scores[o0 + r];
        const bool ok = (!a.labels || a.labels[o0 + r] == a.label) && (!a.score_test || s > a.score_thr);
        pass |= (int)ok << (r - r0);
    }
    int m;
    int pos = block_scan(__popc(pass), sw, m);
    for (int r = r0; r < r0 + per && r < n; ++r) {
        if (!((pass >> (r - r0)) & 1)) continue;
        if (a.nms) skey[pos] = score_key(a.scores[o0 + r], (uint32_t)r);
        else keep[pos] = r;
        ++pos;
    }
    if (!a.nms) {
        for (int p = m + tid; p < n; p += kBoxThreads) keep[p] = -1;
        if (tid == 0) a.count[img] = m;
        return;
    }

    // 2. stable sort by descending score: bitonic over the keys padded to a power of two (padding sorts last)
    int np = 1;
    while (np < m) np <<= 1;
    for (int p = m + tid; p < np; p += kBoxThreads) skey[p] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (np >> 1); i += kBoxThreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const uint64_t x = skey[lo], y = skey[hi];
                if ((x > y) == ((lo & k) == 0)) skey[lo] = y, skey[hi] = x;
            }
            __syncthreads();
        }
    }

    // 3. stage the boxes in score order
    for (int p = tid; p < m; p += kBoxThreads) {
        const int r = (int)(uint32_t)skey[p];
        sbox[p] = *reinterpret_cast<const float4*>(a.boxes + (o0 + r) * 4);
        sdead[p] = 0;
    }
    __syncthreads();

    // 4. greedy sweep in tiles of 64: wave 0 resolves the tile serially with a wave-uniform alive mask, then every thread
    //    suppresses the later boxes against the tile's survivors
    const float thr = a.iou_thr;
    const int lane = tid & 63;
    for (int t0 = 0; t0 < m; t0 += kTile) {
        if (tid < 64) {
            const int p = t0 + lane;
            const bool valid = p < m;
            const float4 bl = valid ? sbox[p] : make_float4(0.f, 0.f, 0.f, 0.f);
            uint64_t alive = __ballot(valid && !sdead[p]);
            for (int k = 0; k < kTile; ++k) {
                if (!((alive >> k) & 1)) continue;   // uniform
                const float4 bk = sbox[t0 + k];
                const bool sup = lane > k && ((alive >> lane) & 1) && box_iou(bk, bl) > thr;
                alive &= ~__ballot(sup);
            }
            if (valid && !((alive >> lane) & 1)) sdead[p] = 1;
            if (lane == 0) *stile = alive;
        }
        __syncthreads();
        const uint64_t alive = *stile;
        for (int p = t0 + kTile + tid; p < m; p += kBoxThreads) {
            if (sdead[p]) continue;
            const float4 bp = sbox[p];
            for (uint64_t s = alive; s; s &= s - 1) {
                if (box_iou(sbox[t0 + __ffsll((unsigned long long)s) - 1], bp) > thr) {
                    sdead[p] = 1;
                    break;
                }
            }
        }
        __syncthreads();
    }

    // 5. compact the survivors in score order
    const int q0 = tid * ((m + kBoxThreads - 1) / kBoxThreads), q1 = min(m, q0 + (m + kBoxThreads - 1) / kBoxThreads);
    int alive_n = 0;
    for (int p = q0; p < q1; ++p) alive_n += !sdead[p];
    int kept;
    int out = block_scan(alive_n, sw, kept);
    for (int p = q0; p < q1; ++p)
        if (!sdead[p]) keep[out++] = (int32_t)(uint32_t)skey[p];
    for (int p = kept + tid; p < n; p += kBoxThreads) keep[p] = -1;
    if (tid == 0) a.count[img] = kept;
}

// Source index and weights of one output coordinate (torch's upsample_bilinear2d, align_corners=True):
// src = scale * dst, i0 = int(src), i1 = i0 + (i0 < n - 1), l1 = src - i0, l0 = 1 - l1.
struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap make_tap(float scale, int dst, int n) {
    const float src = scale * (float)dst;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// One workgroup per (b, j) map.  LDS: the H x W source map | row taps [Ho] (offsets pre-multiplied by W) | column taps [Wo].
__global__ __launch_bounds__(256) void resize_argmax_kernel(const float* __restrict__ hm, int H, int W, int Ho, int Wo, float sh,
                                                            float sw, int32_t* idx, float* maxval, float* preds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int hw = H * W;
    float* smap = reinterpret_cast<float*>(smem);
    Tap* rows = reinterpret_cast<Tap*>(smem + (((size_t)hw * 4 + 15) & ~(size_t)15));
    Tap* cols = rows + Ho;
    __shared__ float sv[4];
    __shared__ int si[4];
    const float* src = hm + (size_t)blockIdx.x * hw;
    if ((hw & 3) == 0) {
        for (int e = threadIdx.x; e < (hw >> 2); e += 256) reinterpret_cast<float4*>(smap)[e] = reinterpret_cast<const float4*>(src)[e];
    } else {
        for (int e = threadIdx.x; e < hw; e += 256) smap[e] = src[e];
    }
    for (int y = threadIdx.x; y < Ho; y += 256) {
        Tap t = make_tap(sh, y, H);
        t.i0 *= W, t.i1 *= W;
        rows[y] = t;
    }
    for (int x = threadIdx.x; x < Wo; x += 256) cols[x] = make_tap(sw, x, W);
    __syncthreads();

    float bv = -INFINITY;
    int bi = 0x7fffffff;
    const int n = Ho * Wo;
    int oy = threadIdx.x / Wo, ox = threadIdx.x - oy * Wo;
    const int dy = 256 / Wo, dx = 256 - dy * Wo;
    const bool same = Ho == H && Wo == W;   // torch copies the input at the identity size (no 0 * inf / NaN from a neighbour)
    for (int e = threadIdx.x; e < n; e += 256) {
        const Tap r = rows[oy], c = cols[ox];
        // W first within each row, then the rows (torch's order)
        const float top = c.l0 * smap[r.i0 + c.i0] + c.l1 * smap[r.i0 + c.i1];
        const float bot = c.l0 * smap[r.i1 + c.i0] + c.l1 * smap[r.i1 + c.i1];
        argmax_take(same ? smap[e] : r.l0 * top + r.l1 * bot, e, bv, bi);
        oy += dy, ox += dx;
        if (ox >= Wo) ox -= Wo, ++oy;
    }
    block_argmax_reduce(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        if (idx) idx[blockIdx.x] = bi;
        maxval[blockIdx.x] = bv;
        const float m = bv > 0.f ? 1.f : 0.f;
        preds[2 * blockIdx.x] = (float)(bi % Wo) * m;
        preds[2 * blockIdx.x + 1] = (float)(bi / Wo) * m;
    }
}

size_t resize_lds(int H, int W, int Ho, int Wo) { return (((size_t)H * W * 4 + 15) & ~(size_t)15) + (size_t)(Ho + Wo) * sizeof(Tap); }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_box_select(const float* boxes, const float* scores, const int64_t* labels, const int64_t* offsets, int num_images,
                              int64_t N, int max_n, int64_t label, int score_test, float score_thr, double iou_thr, int32_t* keep,
                              int32_t* count, void* stream) {
    STL_CHECK(num_images >= 0 && N >= 0 && N < (1ll << 31), "box_select: %d images, N = %lld", num_images, (long long)N);
    STL_CHECK(max_n >= 0 && max_n <= STL_BOX_MAX, "box_select: max_n = %d (at most %d boxes per image)", max_n, STL_BOX_MAX);
    if (num_images == 0) return 0;
    STL_CHECK(offsets && count && (N == 0 || (boxes && scores && keep)), "box_select: null pointer");
    const int mn = max_n > 0 ? max_n : 1;
    int cap = 1;
    while (cap < mn) cap <<= 1;
    // torchvision compares the float IoU with a double threshold: iou > t  <=>  iou > (the largest float <= t)
    float thr = (float)iou_thr;
    if ((double)thr > iou_thr) thr = nextafterf(thr, -INFINITY);
    const size_t lds = (size_t)cap * 8 + (size_t)mn * 16 + ((mn + 15) & ~15) + kBoxWaves * 4 + 8;
    hipFuncSetAttribute(reinterpret_cast<const void*>(&box_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const BoxArgs a{boxes, scores, labels, offsets, N, label, score_thr, thr, keep, count, mn, cap, iou_thr >= 0.0, score_test != 0};
    STL_LAUNCH(box_select_kernel, dim3(num_images), dim3(kBoxThreads), lds, ST, a);
    STL_LAUNCH_CHECK("box_select");
    return 0;
}

extern "C" int stl_heatmap_resize_argmax(const float* hm, int BJ, int H, int W, int Ho, int Wo, int32_t* idx, float* maxval,
                                         float* preds, void* stream) {
    STL_CHECK(BJ >= 0 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "heatmap_resize_argmax: %d maps of %d x %d -> %d x %d", BJ, H, W,
              Ho, Wo);
    STL_CHECK((int64_t)H * W <= STL_RESIZE_SRC_MAX, "heatmap_resize_argmax: a %d x %d map (H * W <= %d)", H, W, STL_RESIZE_SRC_MAX);
    STL_CHECK(Ho <= STL_RESIZE_DST_MAX && Wo <= STL_RESIZE_DST_MAX, "heatmap_resize_argmax: output %d x %d (each side <= %d)", Ho, Wo,
              STL_RESIZE_DST_MAX);
    if (BJ == 0) return 0;
    STL_CHECK(hm && maxval && preds, "heatmap_resize_argmax: null pointer");
    // area_pixel_compute_scale with align_corners: (in - 1) / (out - 1) in float, 0 for a single output row / column
    const float sh = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    const float sw = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    // the dynamic LDS this launch needs (the kernel's static LDS comes on top: asking for all 160 KiB would be refused)
    const size_t lds = resize_lds(H, W, Ho, Wo);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&resize_argmax_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    STL_LAUNCH(resize_argmax_kernel, dim3(BJ), dim3(256), lds, ST, hm, H, W, Ho, Wo, sh, sw, idx, maxval, preds);
    STL_LAUNCH_CHECK("heatmap_resize_argmax");
    return 0;
}
