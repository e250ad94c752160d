// The new pieces of an EfficientNet MBConv block's backward on gfx950 (stlpose_amd/detector_train.py,
// include/stlpose_hip_det_mbconv.h): the squeeze-excitation gate, the gated projection's input and the bias gradient of the
// depthwise layer's folded BN.  NHWC, fp32.  The forward (detector.hip) keeps the block's maps a = swish(u) and g = the gate; the
// pre-activation u is recomputed by the caller with the forward's own launch.
//
//   stl_det_mbconv_gate_bwd  gate_bwd_kernel   one workgroup per (64 V channels, pixel range, image), V = 4 channels per thread
//                                              (1 where C % 4 != 0): lane -> channels, wave -> every fourth pixel of the range;
//                                              xs = a g, and the range's sums of a and of D a (a thread adds its pixels in order,
//                                              then the four waves in wave order through LDS)
//                            gate_sum_kernel   asum / dgate: an image's ranges added in range order, fp64, rounded once
//   stl_det_se_bwd           se_bwd_image_kernel   one workgroup per image, the layout of se_kernel in detector.hip: p, r, q with the
//                                              forward's expressions, dv, dq, dr, dpool; p, dv, q, dr go to the workspace
//                            se_bwd_weight_kernel  dw2, db2, dw1, db1: one thread per element, the images added in order
//   stl_det_mbconv_act_bwd   act_bwd_kernel    gate_bwd_kernel's decomposition: du = (D g + dpool / HW) swish'(u) and the range's sum
//                            act_sum_kernel    db: the (image, range) partial sums added in that order, fp64, rounded once
//
// Streaming kernels, bound by memory bandwidth; LDS only for the wave sums.  Every reduction runs in a fixed order (no float
// atomics): two runs give bitwise equal results.  Generic in C and Cs (1152 / 48 for D0; 1392 / 58 and 2304 / 96 for D3).
#include "common.cuh"
#include "../../include/stlpose_hip_det_mbconv.h"

namespace {

// the forward's swish (detector.hip) and swish'(z) = s (1 + z (1 - s)), s = sigmoid(z) (detector_train.hip)
__device__ __forceinline__ float swishf(float x) { return x * (1.f / (1.f + __expf(-x))); }
__device__ __forceinline__ float dswishf(float z) {
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
}

constexpr int kPartsMax = 16, kPartPix = 16;   // at most 16 pixel ranges per image, of at least 16 pixels
// Above 1024 pixels (the blocks in front of the final stage: up to 256 x 256) ranges of 64 pixels, at most 1024 of them: a thread's
// fp32 chain stays 16 terms long -- with 16 ranges it would be 1024 terms at 256 x 256, and the sums' error several times that of a
// pairwise sum -- and the ranges are added in fp64.
constexpr int kLargeHW = 1024, kLargePartPix = 64, kLargePartsMax = 1024;
static inline int parts_of(int HW) {
    if (HW > kLargeHW) {
        const int p = (HW + kLargePartPix - 1) / kLargePartPix;
        return p > kLargePartsMax ? kLargePartsMax : p;
    }
    const int p = (HW + kPartPix - 1) / kPartPix;
    return p < 1 ? 1 : (p > kPartsMax ? kPartsMax : p);
}

template <int V>
__device__ __forceinline__ void load(const float* p, float* v) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void store(float* p, const float* v) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// grid (ceil(C / 64 V), parts, B); range `sp` holds pixels [sp * per, min(HW, (sp + 1) * per)); partial [B][parts][2][C]
template <int V>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ a, const float* __restrict__ D, const float* __restrict__ g,
                                                       float* __restrict__ xs, float* __restrict__ partial, int HW, int C, int per) {
    __shared__ float red[2][4][64 * V];
    const int b = blockIdx.z, sp = blockIdx.y, parts = gridDim.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * V;   // C % V == 0: c < C means c + V <= C
    const int p0 = sp * per, p1 = min(HW, p0 + per);
    float sa[V], sd[V];
#pragma unroll
    for (int k = 0; k < V; ++k) sa[k] = sd[k] = 0.f;
    if (c < C) {
        float gv[V];
        load<V>(g + (int64_t)b * C + c, gv);
        for (int p = p0 + wv; p < p1; p += 4) {
            const int64_t off = ((int64_t)b * HW + p) * C + c;
            float av[V], dv[V], xv[V];
            load<V>(a + off, av);
            load<V>(D + off, dv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                xv[k] = av[k] * gv[k];
                sa[k] += av[k];
                sd[k] += dv[k] * av[k];
            }
            store<V>(xs + off, xv);
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) red[0][wv][lane * V + k] = sa[k], red[1][wv][lane * V + k] = sd[k];
    __syncthreads();
    if (wv == 0 && c < C) {
        float* o = partial + ((int64_t)b * parts + sp) * 2 * C + c;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int i = lane * V + k;
            o[k] = ((red[0][0][i] + red[0][1][i]) + red[0][2][i]) + red[0][3][i];
            o[C + k] = ((red[1][0][i] + red[1][1][i]) + red[1][2][i]) + red[1][3][i];
        }
    }
}

// one thread per (image, channel)
__global__ __launch_bounds__(256) void gate_sum_kernel(const float* __restrict__ partial, int parts, int B, int C, float* __restrict__ asum,
                                                       float* __restrict__ dgate) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * C) return;
    const int c = (int)(e % C);
    const int64_t b = e / C;
    double s0 = 0.0, s1 = 0.0;
    for (int sp = 0; sp < parts; ++sp) {
        const float* q = partial + (b * parts + sp) * 2 * C + c;
        s0 += (double)q[0];
        s1 += (double)q[C];
    }
    asum[e] = (float)s0;
    dgate[e] = (float)s1;
}

// D and du may be the same array: a thread reads its elements of D before it writes them.  partial [B][parts][C]
template <int V>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* D, const float* __restrict__ u, const float* __restrict__ g,
                                                      const float* __restrict__ dpool, float* du, float* __restrict__ partial, int HW, int C,
                                                      int per) {
    __shared__ float red[4][64 * V];
    const int b = blockIdx.z, sp = blockIdx.y, parts = gridDim.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * V;
    const int p0 = sp * per, p1 = min(HW, p0 + per);
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    if (c < C) {
        float gv[V], pm[V];
        load<V>(g + (int64_t)b * C + c, gv);
        load<V>(dpool + (int64_t)b * C + c, pm);
#pragma unroll
        for (int k = 0; k < V; ++k) pm[k] = pm[k] / (float)HW;
        for (int p = p0 + wv; p < p1; p += 4) {
            const int64_t off = ((int64_t)b * HW + p) * C + c;
            float dv[V], uv[V], o[V];
            load<V>(D + off, dv);
            load<V>(u + off, uv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                o[k] = (dv[k] * gv[k] + pm[k]) * dswishf(uv[k]);
                acc[k] += o[k];
            }
            store<V>(du + off, o);
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) red[wv][lane * V + k] = acc[k];
    __syncthreads();
    if (wv == 0 && c < C) {
        float* o = partial + ((int64_t)b * parts + sp) * C + c;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int i = lane * V + k;
            o[k] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
        }
    }
}

// one thread per channel: the n = B * parts partial sums in order
__global__ __launch_bounds__(256) void act_sum_kernel(const float* __restrict__ partial, int n, int C, float* __restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += (double)partial[(int64_t)j * C + c];
    db[c] = (float)s;
}

// HW above kLargeHW (up to 1024 ranges per image: one thread per channel over all B * parts would be a chain of 32768 loads): first one
// thread per (image, channel) adds the image's ranges in range order, fp64, and leaves the sum as a float pair (hi, lo) in the image's
// first two ranges -- it alone reads or writes that column of that image --, then one thread per channel adds the images in order
__global__ __launch_bounds__(256) void act_sum_image_kernel(float* partial, int parts, int B, int C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * C) return;
    float* q = partial + (e / C) * parts * C + e % C;
    double s = 0.0;
    for (int sp = 0; sp < parts; ++sp) s += (double)q[(int64_t)sp * C];
    const float hi = (float)s;
    q[0] = hi;
    q[C] = (float)(s - (double)hi);
}

__global__ __launch_bounds__(256) void act_sum_images_kernel(const float* __restrict__ partial, int parts, int B, int C,
                                                             float* __restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* q = partial + (int64_t)b * parts * C + c;
        s += (double)q[0] + (double)q[C];
    }
    db[c] = (float)s;
}

// one workgroup per image; LDS: p [C] | dv [C] | r [Cs] | dr [Cs]; ws [B][p C | dv C | q Cs | dr Cs]
__global__ __launch_bounds__(256) void se_bwd_image_kernel(const float* __restrict__ asum, const float* __restrict__ dgate,
                                                           const float* __restrict__ g, int HW, int C, int Cs, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           float* __restrict__ ws, float* __restrict__ dpool) {
    extern __shared__ float sm[];
    float* p = sm;
    float* dv = sm + C;
    float* r = sm + 2 * C;
    float* dr = r + Cs;
    const int b = blockIdx.x;
    float* wp = ws + (int64_t)b * (2 * C + 2 * Cs);
    for (int c = threadIdx.x; c < C; c += 256) {
        const int64_t e = (int64_t)b * C + c;
        const float gg = g[e];
        p[c] = asum[e] / (float)HW;
        dv[c] = dgate[e] * (gg * (1.f - gg));
        wp[c] = p[c];
        wp[C + c] = dv[c];
    }
    __syncthreads();
    // as se_kernel: one wave per hidden unit, lanes stride over C, then a fixed-order wave reduction
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j = wv; j < Cs; j += 4) {
        float acc = 0.f, dq = 0.f;
        for (int c = lane; c < C; c += 64) {
            acc += w1[(int64_t)j * C + c] * p[c];
            dq += w2[(int64_t)c * Cs + j] * dv[c];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o), dq += __shfl_xor(dq, o);
        if (lane == 0) {
            const float rj = acc + b1[j];
            r[j] = rj;
            dr[j] = dq * dswishf(rj);
            wp[2 * C + j] = swishf(rj);
            wp[2 * C + Cs + j] = dr[j];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < Cs; ++j) acc += w1[(int64_t)j * C + c] * dr[j];
        dpool[(int64_t)b * C + c] = acc;
    }
}

// element e of dw2 [C][Cs] and of dw1 [Cs][C], and of db2 / db1 where e < C / Cs; the images in order
__global__ __launch_bounds__(256) void se_bwd_weight_kernel(const float* __restrict__ ws, int B, int C, int Cs, float* __restrict__ dw1,
                                                            float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)C * Cs, st = 2 * C + 2 * Cs;
    if (e >= n) return;
    {
        const int c = (int)(e / Cs), j = (int)(e % Cs);
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += ws[b * st + C + c] * ws[b * st + 2 * C + j];
        dw2[e] = acc;
    }
    {
        const int j = (int)(e / C), c = (int)(e % C);
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += ws[b * st + 2 * C + Cs + j] * ws[b * st + c];
        dw1[e] = acc;
    }
    if (e < C) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += ws[b * st + C + e];
        db2[e] = acc;
    }
    if (e < Cs) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += ws[b * st + 2 * C + Cs + e];
        db1[e] = acc;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_det_mbconv_parts(int HW) { return HW >= 1 ? parts_of(HW) : 0; }

extern "C" int64_t stl_det_mbconv_gate_bwd_workspace(int B, int HW, int C) {
    return B >= 1 && HW >= 1 && C >= 1 ? (int64_t)B * parts_of(HW) * 2 * C : 0;
}

extern "C" int stl_det_mbconv_gate_bwd(const float* a, const float* D, const float* g, float* xs, float* partial, float* asum, float* dgate,
                                       int B, int HW, int C, void* stream) {
    STL_CHECK(a && D && g && xs && partial && asum && dgate, "det_mbconv_gate_bwd: null pointer");
    STL_CHECK(B >= 1 && HW >= 1 && C >= 1, "det_mbconv_gate_bwd: B %d HW %d C %d", B, HW, C);
    STL_CHECK(B <= 65535 && HW <= (1 << 26) && ((int64_t)B * C + 255) / 256 < (1ll << 31), "det_mbconv_gate_bwd: B %d HW %d C %d too large", B,
              HW, C);
    const int64_t n = (int64_t)B * HW * C;
    STL_CHECK(((uintptr_t)xs + 4 * (uintptr_t)n <= (uintptr_t)a || (uintptr_t)a + 4 * (uintptr_t)n <= (uintptr_t)xs) &&
                  ((uintptr_t)xs + 4 * (uintptr_t)n <= (uintptr_t)D || (uintptr_t)D + 4 * (uintptr_t)n <= (uintptr_t)xs),
              "det_mbconv_gate_bwd: xs overlaps a or D");
    const int parts = parts_of(HW), per = (HW + parts - 1) / parts;
    const bool vec = C % 4 == 0 && al16(a) && al16(D) && al16(g) && al16(xs);
    if (vec) {
        STL_LAUNCH(gate_bwd_kernel<4>, dim3((unsigned)((C / 4 + 63) / 64), parts, B), dim3(256), 0, ST, a, D, g, xs, partial, HW, C, per);
    } else {
        STL_LAUNCH(gate_bwd_kernel<1>, dim3((unsigned)((C + 63) / 64), parts, B), dim3(256), 0, ST, a, D, g, xs, partial, HW, C, per);
    }
    STL_LAUNCH_CHECK("det_mbconv_gate_bwd");
    STL_LAUNCH(gate_sum_kernel, dim3((unsigned)(((int64_t)B * C + 255) / 256)), dim3(256), 0, ST, (const float*)partial, parts, B, C, asum,
               dgate);
    STL_LAUNCH_CHECK("det_mbconv_gate_bwd");
    return 0;
}

extern "C" int64_t stl_det_se_bwd_workspace(int B, int C, int Cs) {
    return B >= 1 && C >= 1 && Cs >= 1 ? (int64_t)B * (2 * (int64_t)C + 2 * (int64_t)Cs) : 0;
}

extern "C" int stl_det_se_bwd(const float* asum, const float* dgate, const float* g, int B, int HW, int C, int Cs, const float* w1,
                              const float* b1, const float* w2, const float* b2, float* workspace, float* dpool, float* dw1, float* db1,
                              float* dw2, float* db2, void* stream) {
    STL_CHECK(asum && dgate && g && w1 && b1 && w2 && b2 && workspace && dpool && dw1 && db1 && dw2 && db2, "det_se_bwd: null pointer");
    STL_CHECK(B >= 1 && HW >= 1 && C >= 1 && Cs >= 1, "det_se_bwd: B %d HW %d C %d Cs %d", B, HW, C, Cs);
    STL_CHECK((int64_t)C + Cs <= 8192, "det_se_bwd: C %d + Cs %d above 8192 (the image kernel keeps 2 C + 2 Cs floats in LDS)", C, Cs);
    STL_CHECK(B <= 65535, "det_se_bwd: B %d too large", B);
    STL_LAUNCH(se_bwd_image_kernel, dim3(B), dim3(256), (size_t)(2 * C + 2 * Cs) * 4, ST, asum, dgate, g, HW, C, Cs, w1, b1, w2, workspace,
               dpool);
    STL_LAUNCH_CHECK("det_se_bwd");
    STL_LAUNCH(se_bwd_weight_kernel, dim3((unsigned)(((int64_t)C * Cs + 255) / 256)), dim3(256), 0, ST, (const float*)workspace, B, C, Cs,
               dw1, db1, dw2, db2);
    STL_LAUNCH_CHECK("det_se_bwd");
    return 0;
}

extern "C" int stl_det_mbconv_act_bwd_parts(int B, int HW) { return B >= 1 && HW >= 1 ? B * parts_of(HW) : 0; }

extern "C" int64_t stl_det_mbconv_act_bwd_workspace(int B, int HW, int C) {
    return B >= 1 && HW >= 1 && C >= 1 ? (int64_t)B * parts_of(HW) * C : 0;
}

extern "C" int stl_det_mbconv_act_bwd(const float* D, const float* u, const float* g, const float* dpool, float* du, float* partial,
                                      float* db, int B, int HW, int C, void* stream) {
    STL_CHECK(D && u && g && dpool && du && partial && db, "det_mbconv_act_bwd: null pointer");
    STL_CHECK(B >= 1 && HW >= 1 && C >= 1, "det_mbconv_act_bwd: B %d HW %d C %d", B, HW, C);
    STL_CHECK(B <= 65535 && HW <= (1 << 26), "det_mbconv_act_bwd: B %d HW %d too large", B, HW);
    const int64_t n = (int64_t)B * HW * C;
    STL_CHECK((uintptr_t)du + 4 * (uintptr_t)n <= (uintptr_t)u || (uintptr_t)u + 4 * (uintptr_t)n <= (uintptr_t)du,
              "det_mbconv_act_bwd: du overlaps u");
    STL_CHECK(du == D || (uintptr_t)du + 4 * (uintptr_t)n <= (uintptr_t)D || (uintptr_t)D + 4 * (uintptr_t)n <= (uintptr_t)du,
              "det_mbconv_act_bwd: du overlaps D without being D");
    const int parts = parts_of(HW), per = (HW + parts - 1) / parts;
    const bool vec = C % 4 == 0 && al16(D) && al16(u) && al16(g) && al16(dpool) && al16(du);
    if (vec) {
        STL_LAUNCH(act_bwd_kernel<4>, dim3((unsigned)((C / 4 + 63) / 64), parts, B), dim3(256), 0, ST, D, u, g, dpool, du, partial, HW, C, per);
    } else {
        STL_LAUNCH(act_bwd_kernel<1>, dim3((unsigned)((C + 63) / 64), parts, B), dim3(256), 0, ST, D, u, g, dpool, du, partial, HW, C, per);
    }
    STL_LAUNCH_CHECK("det_mbconv_act_bwd");
    if (HW > kLargeHW) {
        // act_sum_image_kernel keeps an image's (hi, lo) pair in its first two ranges: HW > kLargeHW gives at least 17
        static_assert((kLargeHW + kLargePartPix) / kLargePartPix >= 2 && kLargePartsMax >= 2, "the two-stage bias sum needs two ranges");
        STL_LAUNCH(act_sum_image_kernel, dim3((unsigned)(((int64_t)B * C + 255) / 256)), dim3(256), 0, ST, partial, parts, B, C);
        STL_LAUNCH_CHECK("det_mbconv_act_bwd");
        STL_LAUNCH(act_sum_images_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ST, (const float*)partial, parts, B, C, db);
    } else {
        STL_LAUNCH(act_sum_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ST, (const float*)partial, B * parts, C, db);
    }
    STL_LAUNCH_CHECK("det_mbconv_act_bwd");
    return 0;
}
