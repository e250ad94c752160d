// What the backward of the WHOLE EfficientNet trunk needs beyond detector_mbconv.hip (stlpose_amd/detector_train.py,
// include/stlpose_hip_det_mbconv.h): the depthwise backward for every kernel size and stride of the backbone (k 3 / 5, s 1 / 2, TF
// "same" padding: same_pad_before of detector.hip) and the stem's weight gradient.  NHWC, fp32.
//
//   stl_det_dwconv_bwd_data_ks    dwconv_bwd_data_ks_kernel<K, S>    gather form, one thread per (input pixel, 4 channels): 16 bytes per
//                                                                    lane, consecutive lanes on consecutive channel quads.  s = 2 visits
//                                                                    only the taps whose parity matches the pixel's ((K + 1) / 2 per axis);
//                                                                    the tap loops are unrolled (at 5 x 5 / 1 the column loop only: 62
//                                                                    VGPRs instead of 206) and a tap outside the map is a select, not
//                                                                    a branch
//   stl_det_dwconv_bwd_weight_ks  dwconv_bwd_weight_ks_kernel<K, S>  one workgroup per (pixel range of the OUTPUT, up to 256 channel
//                                                                    quads): a thread owns one quad and every P-th pixel of the range, P =
//                                                                    256 / quads, K K float4 accumulators in registers (100 VGPRs at k = 5,
//                                                                    no scratch); the P pixel lanes are added in lane order through LDS, one
//                                                                    kernel row per round
//                                 parts_sum_kernel                   the ranges' partial sums added in range order
//   stl_det_stem_bwd              stem_bwd_kernel                    the same decomposition with one output channel per thread (Co is 32 /
//                                                                    40): z recomputed from the canvas with the forward's expression (27
//                                                                    multiply-adds, the 27 weights in registers), dz = dy swish'(z), 27 + 1
//                                                                    accumulators
//
// Streaming kernels, bound by memory bandwidth.  Every sum runs in a fixed order (no float atomics): two runs give bitwise equal results.
#include "common.cuh"
#include "../../include/stlpose_hip_det_mbconv.h"

namespace {

// swish'(z) = s (1 + z (1 - s)), s = sigmoid(z) (detector_train.hip)
__device__ __forceinline__ float dswishf(float z) {
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
}

// TensorFlow "same" padding before the first row / column (detector.hip)
static inline int same_pad_before(int n, int k, int s) {
    const int extra = ((n + s - 1) / s - 1) * s - n + k;
    return (extra > 0 ? extra : 0) / 2;
}

constexpr int kKsPartMax = 1024, kKsPartPix = 128;   // at most 1024 pixel ranges, of at least 128 output pixels
static inline int ks_parts(int64_t npix) {
    const int64_t p = (npix + kKsPartPix - 1) / kKsPartPix;
    return (int)(p < 1 ? 1 : (p > kKsPartMax ? kKsPartMax : p));
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void fma4(float4& a, const float4& x, const float4& y) {
    a.x += x.x * y.x, a.y += x.y * y.y, a.z += x.z * y.z, a.w += x.w * y.w;
}
__device__ __forceinline__ void add4(float4& a, const float4& x) { a.x += x.x, a.y += x.y, a.z += x.z, a.w += x.w; }

// The forward: y[oy] takes x[oy S - py + ky] w[ky], so dx[y] = sum over the ky with (y + py - ky) % S == 0 of dy[(y + py - ky) / S] w[ky]:
// ky = ry + S j with ry = (y + py) % S, output row oy0 - j with oy0 = (y + py - ry) / S; the columns alike.
template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_bwd_data_ks_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                 const float* __restrict__ z, float* __restrict__ dx, int B, int H, int W,
                                                                 int C, int Ho, int Wo, int py, int px) {
    constexpr int J = S == 1 ? K : (K + 1) / 2, ROWS = J > 3 ? 1 : J;   // rows unrolled
    const int nq = C >> 2;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * H * W * nq) return;
    const int c = (int)(e % nq) * 4;
    const int64_t pix = e / nq;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    const int ry = S == 1 ? 0 : (y + py) & 1, rx = S == 1 ? 0 : (x + px) & 1;
    const int oy0 = (y + py - ry) / S, ox0 = (x + px - rx) / S;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // the row loop stays a loop at 5 x 5 / 1: unrolled, all 25 taps' loads are in flight (206 VGPRs, 2 waves per SIMD); a row's are enough
#pragma unroll ROWS
    for (int j = 0; j < J; ++j) {
        const int ky = ry + S * j, oy = oy0 - j;
        const bool oky = ky < K && oy >= 0 && oy < Ho;
#pragma unroll
        for (int i = 0; i < J; ++i) {
            const int kx = rx + S * i, ox = ox0 - i;
            const bool ok = oky && kx < K && ox >= 0 && ox < Wo;
            // a tap outside reads element c of the first pixel and of the first tap, and is dropped
            const int64_t o = ok ? ((b * Ho + oy) * Wo + ox) * C + c : c;
            const int t = ok ? ky * K + kx : 0;
            float4 g = ld4(dy + o);
            const float4 wv = ld4(w + (int64_t)t * C + c);
            if (!ok) g = make_float4(0.f, 0.f, 0.f, 0.f);
            fma4(acc, g, wv);
        }
    }
    const int64_t off = pix * C + c;
    if (z) {
        const float4 zv = ld4(z + off);
        acc.x *= dswishf(zv.x), acc.y *= dswishf(zv.y), acc.z *= dswishf(zv.z), acc.w *= dswishf(zv.w);
    }
    *reinterpret_cast<float4*>(dx + off) = acc;
}

// grid (parts, ceil(quads / 256)); nqb = min(quads, 256) quads per workgroup, P = 256 / nqb pixel lanes; range `part` holds the output
// pixels [part * per, min(npix, (part + 1) * per)); partial [parts][K K][C]
template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_bwd_weight_ks_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   float* __restrict__ partial, int64_t npix, int H, int W, int C, int Ho,
                                                                   int Wo, int py, int px, int64_t per, int nqb) {
    __shared__ float4 red[K][256];
    const int nq = C >> 2, P = 256 / nqb;
    const int t = threadIdx.x, ql = t % nqb, pl = t / nqb;
    const int q = blockIdx.y * nqb + ql;
    const int c = q * 4;
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    float4 acc[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pl < P && q < nq) {
        for (int64_t p = p0 + pl; p < p1; p += P) {
            const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
            const int64_t b = p / ((int64_t)Wo * Ho);
            const float4 g = ld4(dy + p * C + c);
            const int iy0 = oy * S - py, ix0 = ox * S - px;
            const int64_t base = ((b * H + iy0) * W + ix0) * C + c;   // may lie in front of the map: used only where the tap is inside
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const bool oky = iy0 + ky >= 0 && iy0 + ky < H;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const bool ok = oky && ix0 + kx >= 0 && ix0 + kx < W;
                    float4 xv = ld4(x + (ok ? base + ((int64_t)ky * W + kx) * C : (int64_t)c));
                    if (!ok) xv = make_float4(0.f, 0.f, 0.f, 0.f);
                    fma4(acc[ky * K + kx], xv, g);
                }
            }
        }
    }
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {   // one kernel row per round: the pixel lanes in lane order
#pragma unroll
        for (int kx = 0; kx < K; ++kx) red[kx][t] = acc[ky * K + kx];
        __syncthreads();
        if (pl == 0 && q < nq) {
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                float4 s = red[kx][ql];
                for (int l = 1; l < P; ++l) add4(s, red[kx][l * nqb + ql]);
                *reinterpret_cast<float4*>(partial + ((int64_t)blockIdx.x * K * K + ky * K + kx) * C + c) = s;
            }
        }
        __syncthreads();
    }
}

// out[e] = sum over parts of partial[part][e], in part order; the first n0 elements go to o0, the rest to o1 (detector_train.hip's
// sum_parts_kernel with an fp64 accumulator)
__global__ __launch_bounds__(256) void parts_sum_kernel(const float* __restrict__ partial, int nparts, int64_t n, int64_t n0,
                                                        float* __restrict__ o0, float* __restrict__ o1) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double acc = 0.0;   // up to 1024 parts: fp64, rounded once
    for (int s = 0; s < nparts; ++s) acc += (double)partial[(int64_t)s * n + e];
    if (e < n0) o0[e] = (float)acc;
    else o1[e - n0] = (float)acc;
}

// grid (parts, ceil(Co / 256)); ncb = min(Co, 256) channels per workgroup, P = 256 / ncb pixel lanes; x [B, H, W, 3], w [3][3][3][Co],
// dy [B, Ho, Wo, Co]; partial [parts][27 Co (dw) | Co (db)]
__global__ __launch_bounds__(256) void stem_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ dy, float* __restrict__ partial, int64_t npix, int H, int W,
                                                       int Ho, int Wo, int Co, int py, int px, int64_t per, int ncb) {
    __shared__ float red[7][256];
    const int P = 256 / ncb;
    const int t = threadIdx.x, cl = t % ncb, pl = t / ncb;
    const int co = blockIdx.y * ncb + cl;
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    float acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.f;
    if (pl < P && co < Co) {
        float wr[27];
#pragma unroll
        for (int i = 0; i < 27; ++i) wr[i] = w[i * Co + co];
        const float bz = bias[co];
        for (int64_t p = p0 + pl; p < p1; p += P) {
            const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
            const int64_t b = p / ((int64_t)Wo * Ho);
            const int iy0 = oy * 2 - py, ix0 = ox * 2 - px;
            float xv[27], zacc = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const bool oky = iy0 + ky >= 0 && iy0 + ky < H;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const bool ok = oky && ix0 + kx >= 0 && ix0 + kx < W;
                    const float* xp = x + (ok ? (((int64_t)b * H + iy0 + ky) * W + ix0 + kx) * 3 : 0);
                    const int i = (ky * 3 + kx) * 3;
                    xv[i] = ok ? xp[0] : 0.f, xv[i + 1] = ok ? xp[1] : 0.f, xv[i + 2] = ok ? xp[2] : 0.f;
                    zacc += xv[i] * wr[i] + xv[i + 1] * wr[i + 1] + xv[i + 2] * wr[i + 2];   // stem_kernel's expression
                }
            }
            const float dz = dy[p * Co + co] * dswishf(zacc + bz);
#pragma unroll
            for (int i = 0; i < 27; ++i) acc[i] += xv[i] * dz;
            acc[27] += dz;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // seven sums per round: the pixel lanes in lane order
#pragma unroll
        for (int i = 0; i < 7; ++i) red[i][t] = acc[r * 7 + i];
        __syncthreads();
        if (pl == 0 && co < Co) {
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                float s = red[i][cl];
                for (int l = 1; l < P; ++l) s += red[i][l * ncb + cl];
                partial[(int64_t)blockIdx.x * 28 * Co + (int64_t)(r * 7 + i) * Co + co] = s;
            }
        }
        __syncthreads();
    }
}

static inline bool apart(const void* a, int64_t na, const void* b, int64_t nb) {   // two float arrays that do not overlap
    return (uintptr_t)a + 4 * (uintptr_t)na <= (uintptr_t)b || (uintptr_t)b + 4 * (uintptr_t)nb <= (uintptr_t)a;
}

}  // namespace

#define ST ((hipStream_t)stream)
#define KS_DISPATCH(kernel, grid, ...)                                                    \
    do {                                                                                  \
        if (k == 3 && s == 1) STL_LAUNCH((kernel<3, 1>), grid, dim3(256), 0, ST, __VA_ARGS__);      \
        else if (k == 3) STL_LAUNCH((kernel<3, 2>), grid, dim3(256), 0, ST, __VA_ARGS__);           \
        else if (s == 1) STL_LAUNCH((kernel<5, 1>), grid, dim3(256), 0, ST, __VA_ARGS__);           \
        else STL_LAUNCH((kernel<5, 2>), grid, dim3(256), 0, ST, __VA_ARGS__);                       \
    } while (0)

extern "C" int stl_det_dwconv_bwd_data_ks(const float* dy, const float* w, const float* z, float* dx, int B, int H, int W, int C, int k,
                                          int s, void* stream) {
    STL_CHECK(dy && w && dx, "det_dwconv_bwd_data_ks: null pointer");
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1, "det_dwconv_bwd_data_ks: B %d, %d x %d, C %d", B, H, W, C);
    STL_CHECK((k == 3 || k == 5) && (s == 1 || s == 2), "det_dwconv_bwd_data_ks: k %d s %d (k in {3, 5}, s in {1, 2})", k, s);
    STL_CHECK(C % 4 == 0, "det_dwconv_bwd_data_ks: C %d (four channels per thread: C %% 4 == 0)", C);
    STL_CHECK(al16(dy) && al16(w) && al16(dx) && (!z || al16(z)), "det_dwconv_bwd_data_ks: a pointer is not 16-byte aligned");
    const int Ho = (H + s - 1) / s, Wo = (W + s - 1) / s;
    const int64_t n = (int64_t)B * H * W * C, no = (int64_t)B * Ho * Wo * C;
    STL_CHECK((n / 4 + 255) / 256 < (1ll << 31), "det_dwconv_bwd_data_ks: too large");
    STL_CHECK(apart(dx, n, dy, no) && apart(dx, n, w, (int64_t)k * k * C), "det_dwconv_bwd_data_ks: dx overlaps dy or w");
    const dim3 grid((unsigned)((n / 4 + 255) / 256));
    KS_DISPATCH(dwconv_bwd_data_ks_kernel, grid, dy, w, z, dx, B, H, W, C, Ho, Wo, same_pad_before(H, k, s), same_pad_before(W, k, s));
    STL_LAUNCH_CHECK("det_dwconv_bwd_data_ks");
    return 0;
}

extern "C" int stl_det_dwconv_bwd_ks_parts(int64_t npix) { return npix >= 1 ? ks_parts(npix) : 0; }

extern "C" int stl_det_dwconv_bwd_weight_ks(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, int C, int k,
                                            int s, void* stream) {
    STL_CHECK(x && dy && partial && dw, "det_dwconv_bwd_weight_ks: null pointer");
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1, "det_dwconv_bwd_weight_ks: B %d, %d x %d, C %d", B, H, W, C);
    STL_CHECK((k == 3 || k == 5) && (s == 1 || s == 2), "det_dwconv_bwd_weight_ks: k %d s %d (k in {3, 5}, s in {1, 2})", k, s);
    STL_CHECK(C % 4 == 0, "det_dwconv_bwd_weight_ks: C %d (four channels per thread: C %% 4 == 0)", C);
    STL_CHECK(al16(x) && al16(dy) && al16(partial), "det_dwconv_bwd_weight_ks: a pointer is not 16-byte aligned");
    const int Ho = (H + s - 1) / s, Wo = (W + s - 1) / s;
    const int64_t npix = (int64_t)B * Ho * Wo, n = (int64_t)k * k * C;
    const int parts = ks_parts(npix), nq = C / 4, nqb = nq < 256 ? nq : 256;
    STL_CHECK(ceil_div(nq, nqb) <= 65535, "det_dwconv_bwd_weight_ks: C %d too large", C);
    STL_CHECK(apart(partial, parts * n, dw, n) && apart(partial, parts * n, x, (int64_t)B * H * W * C) && apart(partial, parts * n, dy, npix * C) &&
                  apart(dw, n, x, (int64_t)B * H * W * C) && apart(dw, n, dy, npix * C),
              "det_dwconv_bwd_weight_ks: partial or dw overlaps another array");
    const int64_t per = (npix + parts - 1) / parts;
    const dim3 grid(parts, ceil_div(nq, nqb));
    KS_DISPATCH(dwconv_bwd_weight_ks_kernel, grid, x, dy, partial, npix, H, W, C, Ho, Wo, same_pad_before(H, k, s), same_pad_before(W, k, s),
                per, nqb);
    STL_LAUNCH_CHECK("det_dwconv_bwd_weight_ks");
    STL_LAUNCH(parts_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float*)partial, parts, n, n, dw, dw);
    STL_LAUNCH_CHECK("det_dwconv_bwd_weight_ks_sum");
    return 0;
}

extern "C" int stl_det_stem_bwd_parts(int64_t npix) { return npix >= 1 ? ks_parts(npix) : 0; }

extern "C" int stl_det_stem_bwd(const float* x, const float* w, const float* bias, const float* dy, float* partial, float* dw, float* db,
                                int B, int H, int W, int Co, void* stream) {
    STL_CHECK(x && w && bias && dy && partial && dw && db, "det_stem_bwd: null pointer");
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && Co >= 1, "det_stem_bwd: B %d, %d x %d, Co %d", B, H, W, Co);
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int64_t npix = (int64_t)B * Ho * Wo, n = 28ll * Co;
    const int parts = ks_parts(npix), ncb = Co < 256 ? Co : 256;
    STL_CHECK(ceil_div(Co, ncb) <= 65535, "det_stem_bwd: Co %d too large", Co);
    STL_CHECK(apart(partial, parts * n, dw, 27ll * Co) && apart(partial, parts * n, db, Co) && apart(dw, 27ll * Co, db, Co) &&
                  apart(partial, parts * n, dy, npix * Co) && apart(dw, 27ll * Co, w, 27ll * Co) && apart(db, Co, bias, Co),
              "det_stem_bwd: partial, dw or db overlaps another array");
    const int64_t per = (npix + parts - 1) / parts;
    STL_LAUNCH(stem_bwd_kernel, dim3(parts, ceil_div(Co, ncb)), dim3(256), 0, ST, x, w, bias, dy, partial, npix, H, W, Ho, Wo, Co,
               same_pad_before(H, 3, 2), same_pad_before(W, 3, 2), per, ncb);
    STL_LAUNCH_CHECK("det_stem_bwd");
    STL_LAUNCH(parts_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float*)partial, parts, n, 27ll * Co, dw, db);
    STL_LAUNCH_CHECK("det_stem_bwd_sum");
    return 0;
}
