// Fine-tuning the EfficientDet heads on gfx950 (stlpose_amd/detector_train.py): the detection loss with its head-output gradients
// and the backward kernels of the shared heads (depthwise 3x3 -> pointwise + frozen BN -> swish, five levels, one header).  The
// reference has no detection loss for its EfficientDet (src/models/EfficientDet.py takes no targets); this is the published
// RetinaNet / EfficientDet loss, restated in tests/detector_train_ref.py.  NHWC; fp32 first, the 16-bit heads further down.
//
//   stl_det_loss                  IoU assignment of every anchor (positive >= 0.5, negative < 0.4, ignored between), focal
//                                 classification + smooth-L1 regression, and dL/dreg, dL/dlogit for the whole batch: one launch
//                                 for the per-anchor work (one workgroup per image: the image's positive count normalises its
//                                 gradients), a second one adds the per-image losses in image order
//   stl_det_pointwise_bwd_data    dX[m, k] = sum_n dY[m, n] W'[k, n] on v_mfma_f32_16x16x4_f32; dY with the forward's output addressing
//   stl_det_pointwise_bwd_weight  dW'[k, n] = sum_m X[m, k] dY[m, n] and db'[n] = sum_m dY[m, n]: M in slabs over workgroups on
//                                 the same MFMA, then a slab sum in slab order
//   stl_det_dwconv_bwd_data       depthwise 3x3 / 1 "same" data gradient (the taps flipped), optionally times swish'(z) of the
//                                 layer below
//   stl_det_dwconv_bwd_weight     dw[ky, kx, c] over batch and pixels: per-workgroup partial sums, then a sum in partial order
//
// The training forward's pointwise launch (stl_det_pointwise_train, swish with its pre-activation kept) is the forward kernel
// itself and lives in detector.hip.  Every reduction runs in a fixed order (no float atomics): two runs give bitwise equal results.
//
// A model with compute_dtype "f16" trains its heads in 16 bit (further down): forward tensors d, z, t in f16, each rounded once from
// its fp32 value; gradients in flight bf16, rounded once when stored; every sum fp32; dW', db', dw fp32.
//   stl_det_pointwise16_bwd_data    dX = dY W'^T on v_mfma_f32_16x16x32_bf16: dY bf16 (a header's fp32 dreg / dlogit rounded in
//                                   registers) straight from global memory, W'^T from a bf16 transposed pack in the forward's tile layout
//   stl_det_pointwise16_bwd_weight  dW' = X^T dY, db' = sum dY on the same MFMA: X (f16) converted to bf16 while staged, both operands
//                                   transposed through LDS (two rows paired in registers), slabs of M added in slab order
//   stl_det_dwconv16_bwd_data / _weight  8 channels per thread and 16-byte accesses; taps and arithmetic fp32, swish'(z) from the stored z
// (stl_det_pointwise16_train, the 16-bit training forward's launch, is pointwise16_kernel in detector.hip.)
#include "common.cuh"

namespace {

// swish'(z) = s (1 + z (1 - s)), s = sigmoid(z)
__device__ __forceinline__ float dswishf(float z) {
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
}

// ------------------------------------------------------------------------------------------------ loss
constexpr int kLossThreads = 1024;
constexpr int kAssignNeg = -1, kAssignIgnore = -2;

// anchor (y1, x1, y2, x2) against gt rows [g0, g1) of (x1, y1, x2, y2, class): the first argmax if its IoU >= 0.5, else negative / ignored
__device__ __forceinline__ int assign_anchor(const float4 an, const float* __restrict__ gt, int g0, int g1) {
    if (g1 <= g0) return kAssignNeg;
    const float area_a = (an.z - an.x) * (an.w - an.y);
    float best = -1.f;
    int bi = g0;
    for (int g = g0; g < g1; ++g) {
        const float x1 = gt[g * 5], y1 = gt[g * 5 + 1], x2 = gt[g * 5 + 2], y2 = gt[g * 5 + 3];
        const float iw = fmaxf(fminf(an.w, x2) - fmaxf(an.y, x1), 0.f);
        const float ih = fmaxf(fminf(an.z, y2) - fmaxf(an.x, y1), 0.f);
        const float inter = iw * ih;
        const float iou = inter / fmaxf(area_a + (x2 - x1) * (y2 - y1) - inter, 1e-8f);
        if (iou > best) best = iou, bi = g;
    }
    return best >= 0.5f ? bi : (best < 0.4f ? kAssignNeg : kAssignIgnore);
}

// x^gamma and its derivative gamma x^(gamma - 1); gamma == 2 (the default) without powf
__device__ __forceinline__ void pow_gamma(float x, float gamma, float& p, float& dp) {
    if (gamma == 2.f) {
        p = x * x, dp = 2.f * x;
    } else {
        p = powf(x, gamma), dp = gamma * powf(x, gamma - 1.f);
    }
}

// block sum in a fixed order: xor-shuffle inside a wave, then the waves in wave order; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* sw) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int k = 0; k < kLossThreads / 64; ++k) t += sw[k];
    return t;
}

// one workgroup per image.  per_image [B][2] = (L_cls,b, L_reg,b); assign [B][A] workspace
__global__ __launch_bounds__(kLossThreads) void det_loss_kernel(const float* __restrict__ reg, const float* __restrict__ cls,
                                                                const float* __restrict__ anchors, const float* __restrict__ gt,
                                                                const int32_t* __restrict__ offsets, int B, int A, int nc, float alpha,
                                                                float gamma, float box_weight, int32_t* __restrict__ assign,
                                                                float* __restrict__ per_image, float* __restrict__ dreg,
                                                                float* __restrict__ dlogit, int32_t* __restrict__ npos_out) {
    __shared__ float sw[kLossThreads / 64];
    const int b = blockIdx.x;
    const int g0 = offsets[b], g1 = offsets[b + 1];
    int32_t* as = assign + (int64_t)b * A;
    float cnt = 0.f;   // positives of this thread: below 2^24, exact in float
    for (int a = threadIdx.x; a < A; a += kLossThreads) {
        const int s = assign_anchor(reinterpret_cast<const float4*>(anchors)[a], gt, g0, g1);
        as[a] = s;
        cnt += s >= 0 ? 1.f : 0.f;
    }
    const int npos = (int)block_sum(cnt, sw);
    const float cscale = 1.f / ((float)B * (float)max(npos, 1));
    const float rscale = npos > 0 ? box_weight / ((float)B * 4.f * (float)npos) : 0.f;
    const float lo = 1e-4f, hi = (float)(1.0 - 1e-4);
    float csum = 0.f, rsum = 0.f;
    for (int a = threadIdx.x; a < A; a += kLossThreads) {
        const int s = as[a];   // written by this thread
        const int64_t row = (int64_t)b * A + a;
        float4 dr = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s == kAssignIgnore) {
            for (int k = 0; k < nc; ++k) dlogit[row * nc + k] = 0.f;
            reinterpret_cast<float4*>(dreg)[row] = dr;
            continue;
        }
        const int pk = s >= 0 ? (int)gt[s * 5 + 4] : -1;
        for (int k = 0; k < nc; ++k) {
            const float p0 = cls[row * nc + k];
            const float p = fminf(fmaxf(p0, lo), hi);
            float term, dp, f, df;
            if (k == pk) {   // alpha (1 - p)^gamma (-log p)
                const float lg = logf(p);
                pow_gamma(1.f - p, gamma, f, df);
                term = -alpha * f * lg;
                dp = alpha * (df * lg - f / p);
            } else {         // (1 - alpha) p^gamma (-log(1 - p))
                const float lg = log1pf(-p);
                pow_gamma(p, gamma, f, df);
                term = -(1.f - alpha) * f * lg;
                dp = (1.f - alpha) * (f / (1.f - p) - df * lg);
            }
            csum += term;
            dlogit[row * nc + k] = (p0 >= lo && p0 <= hi) ? dp * p0 * (1.f - p0) * cscale : 0.f;   // torch.clamp's gradient mask
        }
        if (s >= 0) {
            const float4 an = reinterpret_cast<const float4*>(anchors)[a];
            const float4 r = reinterpret_cast<const float4*>(reg)[row];
            const float wa = an.w - an.y, ha = an.z - an.x;
            const float cxa = an.y + 0.5f * wa, cya = an.x + 0.5f * ha;
            const float x1 = gt[s * 5], y1 = gt[s * 5 + 1], x2 = gt[s * 5 + 2], y2 = gt[s * 5 + 3];
            const float cxg = x1 + 0.5f * (x2 - x1), cyg = y1 + 0.5f * (y2 - y1);
            const float wg = fmaxf(x2 - x1, 1.f), hg = fmaxf(y2 - y1, 1.f);
            const float t[4] = {(cyg - cya) / ha, (cxg - cxa) / wa, logf(hg / ha), logf(wg / wa)};
            const float rv[4] = {r.x, r.y, r.z, r.w};
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float diff = t[j] - rv[j], d = fabsf(diff);
                const bool quad = d <= 1.f / 9.f;
                rsum += quad ? 4.5f * d * d : d - 1.f / 18.f;
                const float dl = quad ? 9.f * d : 1.f;
                g[j] = (diff > 0.f ? -dl : (diff < 0.f ? dl : 0.f)) * rscale;
            }
            dr = make_float4(g[0], g[1], g[2], g[3]);
        }
        reinterpret_cast<float4*>(dreg)[row] = dr;
    }
    const float ctot = block_sum(csum, sw), rtot = block_sum(rsum, sw);
    if (threadIdx.x == 0) {
        per_image[b * 2] = ctot / (float)max(npos, 1);
        per_image[b * 2 + 1] = npos > 0 ? rtot / (4.f * (float)npos) : 0.f;
        npos_out[b] = npos;
    }
}

// losses[0] = mean_b L_cls,b, losses[1] = box_weight * mean_b L_reg,b, added in image order
__global__ void det_loss_finish_kernel(const float* __restrict__ per_image, int B, float box_weight, float* __restrict__ losses) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float c = 0.f, r = 0.f;
    for (int b = 0; b < B; ++b) c += per_image[b * 2], r += per_image[b * 2 + 1];
    losses[0] = c / (float)B;
    losses[1] = box_weight * (r / (float)B);
}

// ------------------------------------------------------------------------------------------------ pointwise backward
constexpr int kT = 64, kStep = 16;   // 64 x 64 output tile per workgroup, 16 of the contracted dimension per LDS stage
constexpr int kSlabMin = 256, kSlabMax = 128;   // bwd_weight: at least 256 rows per slab, at most 128 slabs

__device__ __forceinline__ int64_t dy_row(const StlDetPointwiseBwd& p, int64_t m) {
    const int64_t img = m / p.HW, pix = m - img * p.HW;
    return img * p.dy_img_stride + pix * p.dy_row_stride + p.dy_off;
}

// dX[m, k] = sum_n dY[m, n] W'[k, n].  Grid (M tiles, Ci tiles); wave w owns rows 16w .. 16w + 15 and 64 k columns.
__global__ __launch_bounds__(256) void pointwise_bwd_data_kernel(const StlDetPointwiseBwd p) {
    __shared__ float sa[kStep][kT + 4];   // [n][m]: dY
    __shared__ float sb[kStep][kT + 4];   // [n][k]: W' transposed
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * kT;
    const int k0 = blockIdx.y * kT;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int sm = tid >> 2, sn = (tid & 3) * 4;   // staging: 64 rows (m for dY, k for W') x 4 consecutive n
    const int64_t arow = m0 + sm;
    const bool arow_ok = arow < p.M;
    const float* dyr = p.dy + (arow_ok ? dy_row(p, arow) : 0);
    const bool brow_ok = k0 + sm < p.Kp;
    const float* wr = p.w + (int64_t)(brow_ok ? k0 + sm : 0) * p.Np;
    for (int n0 = 0; n0 < p.Co; n0 += kStep) {   // n0 + 16 <= Np: the packed rows are zero past Co
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + sn + q;
            sa[sn + q][sm] = (arow_ok && n < p.Co) ? dyr[n] : 0.f;
        }
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (brow_ok) w4 = *reinterpret_cast<const float4*>(wr + n0 + sn);
        sb[sn][sm] = w4.x, sb[sn + 1][sm] = w4.y, sb[sn + 2][sm] = w4.z, sb[sn + 3][sm] = w4.w;
        __syncthreads();
#pragma unroll
        for (int ns = 0; ns < kStep; ns += 4) {
            const float a = sa[ns + (lane >> 4)][wv * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bv = sb[ns + (lane >> 4)][j * 16 + (lane & 15)];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + j * 16 + (lane & 15);
        if (k >= p.Ci) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + wv * 16 + (lane >> 4) * 4 + r;
            if (m < p.M) p.dx[m * p.Ci + k] = acc[j][r];
        }
    }
}

static inline int64_t slab_rows(int64_t M) {
    const int64_t per = (M + kSlabMax - 1) / kSlabMax;
    const int64_t r = (per + kStep - 1) / kStep * kStep;
    return r < kSlabMin ? kSlabMin : r;
}

// partial[slab][Ci * Co + Co]: dW' [Ci][Co] of the slab's rows, then db' [Co].  Grid (slabs, Ci tiles, Co tiles); wave w owns
// k rows 16w .. 16w + 15 and 64 n columns; the Ci-tile-0 workgroups also add db' (thread n < 64, rows in order).
__global__ __launch_bounds__(256) void pointwise_bwd_weight_kernel(const StlDetPointwiseBwd p, int64_t rows) {
    __shared__ float sx[kStep][kT + 4];   // [m][k]
    __shared__ float sy[kStep][kT + 4];   // [m][n]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k0 = blockIdx.y * kT, n0 = blockIdx.z * kT;
    const int64_t mbeg = (int64_t)blockIdx.x * rows;
    const int64_t mend = mbeg + rows < p.M ? mbeg + rows : p.M;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f;
    const int sm = tid >> 4, sc = (tid & 15) * 4;   // staging: 16 rows x 4 consecutive columns
    for (int64_t ms = mbeg; ms < mend; ms += kStep) {
        const int64_t row = ms + sm;
        const bool ok = row < mend;
        const float* xr = p.x + (ok ? row : 0) * (int64_t)p.Ci;
        const float* dyr = p.dy + (ok ? dy_row(p, row) : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + sc + q, n = n0 + sc + q;
            sx[sm][sc + q] = (ok && k < p.Ci) ? xr[k] : 0.f;
            sy[sm][sc + q] = (ok && n < p.Co) ? dyr[n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kStep; s += 4) {
            const float a = sx[s + (lane >> 4)][wv * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bv = sy[s + (lane >> 4)][j * 16 + (lane & 15)];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[j], 0, 0, 0);
            }
        }
        if (blockIdx.y == 0 && tid < kT) {
#pragma unroll
            for (int s = 0; s < kStep; ++s) bacc += sy[s][tid];
        }
        __syncthreads();
    }
    float* part = p.partial + (int64_t)blockIdx.x * ((int64_t)p.Ci * p.Co + p.Co);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (n >= p.Co) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + wv * 16 + (lane >> 4) * 4 + r;
            if (k < p.Ci) part[(int64_t)k * p.Co + n] = acc[j][r];
        }
    }
    if (blockIdx.y == 0 && tid < kT && n0 + tid < p.Co) part[(int64_t)p.Ci * p.Co + n0 + tid] = bacc;
}

// out[e] = sum over parts of partial[part][e], in part order; the first n0 elements go to o0, the rest to o1
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ partial, int nparts, int64_t n, int64_t n0,
                                                        float* __restrict__ o0, float* __restrict__ o1) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float acc = 0.f;
    for (int s = 0; s < nparts; ++s) acc += partial[(int64_t)s * n + e];
    if (e < n0) o0[e] = acc;
    else o1[e - n0] = acc;
}

// ------------------------------------------------------------------------------------------------ depthwise backward
// dX[b, y, x, c] = sum_{ky, kx} dY[b, y + 1 - ky, x + 1 - kx, c] w[ky][kx][c] (the forward's taps, flipped), times swish'(z) if z
__global__ __launch_bounds__(256) void dwconv_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                              const float* __restrict__ z, float* __restrict__ dx, int B, int H, int W,
                                                              int C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * H * W * C) return;
    const int c = (int)(e % C);
    const int64_t pix = e / C;
    const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int oy = y + 1 - ky;
        if (oy < 0 || oy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ox = x + 1 - kx;
            if (ox < 0 || ox >= W) continue;
            acc += dy[(((int64_t)b * H + oy) * W + ox) * C + c] * w[(ky * 3 + kx) * C + c];
        }
    }
    dx[e] = z ? acc * dswishf(z[e]) : acc;
}

constexpr int kDwPartMax = 256, kDwPartPix = 256;   // at most 256 partial sums, at least 256 pixels each
static inline int dw_parts(int64_t npix) {
    const int64_t p = (npix + kDwPartPix - 1) / kDwPartPix;
    return (int)(p < 1 ? 1 : (p > kDwPartMax ? kDwPartMax : p));
}

// partial[part][9][C]: a workgroup is 64 channels x 4 pixel lanes (one wave each) over the part's pixels; a thread adds its pixels
// in pixel order, then the 4 lanes are added in lane order
__global__ __launch_bounds__(256) void dwconv_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                float* __restrict__ partial, int64_t npix, int H, int W, int C,
                                                                int64_t per) {
    __shared__ float red[4][9][64];
    const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    float acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.f;
    if (c < C) {
        for (int64_t p = p0 + pl; p < p1; p += 4) {
            const int px = (int)(p % W), py = (int)((p / W) % H);
            const float g = dy[p * C + c];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = py - 1 + ky;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = px - 1 + kx;
                    if (ix < 0 || ix >= W) continue;
                    acc[ky * 3 + kx] += x[(p + (int64_t)(ky - 1) * W + (kx - 1)) * C + c] * g;
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) red[pl][t][cl] = acc[t];
    __syncthreads();
    if (pl == 0 && c < C) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
            partial[((int64_t)blockIdx.x * 9 + t) * C + c] = ((red[0][t][cl] + red[1][t][cl]) + red[2][t][cl]) + red[3][t][cl];
    }
}

// ================================================================================================ 16-bit heads (compute_dtype "f16")
// The backward of a 16-bit head.  Forward tensors (d, z, t) are stored in the model's 16-bit type, gradients in flight are bf16
// (rounded once when stored), every sum is fp32, and dW', db', dw come out in fp32 as in the fp32 path.  Both pointwise kernels run
// on v_mfma_f32_16x16x32_bf16.

// 8 consecutive n of dY row m as a bf16 MFMA operand: bf16 [.., Co] straight (Co % 8 == 0), or a header's fp32 dreg / dlogit
// rounded to bf16 in registers (any Co, any offset: element loads).  Zero past Co.
__device__ __forceinline__ V16 load_dy8(const StlDetPointwise16Bwd& p, int64_t base, int n) {
    if (n >= p.Co) return zero16();
    if (!p.dy_f32) return ldg16(reinterpret_cast<const __bf16*>(p.dy) + base + n);
    const float* r = reinterpret_cast<const float*>(p.dy) + base + n;
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = n + i < p.Co ? r[i] : 0.f;
    return pack<__bf16>(f);
}

__device__ __forceinline__ int64_t dy_row16(const StlDetPointwise16Bwd& p, int64_t m) {
    const int64_t img = m / p.HW, pix = m - img * p.HW;
    return img * p.dy_img_stride + pix * p.dy_row_stride + p.dy_off;
}

// dX[m, k] = sum_n dY[m, n] W'[k, n]: the forward's GEMM (detector.hip, pointwise16_kernel) with dY in the place of x and the bf16
// transposed pack wt [Np / 16][Kp / 32][64][8] (Np over Ci, Kp over Co) in the place of w; no LDS.  A wave owns 32 rows x 64 k,
// a lane ends up with 4 consecutive k of one row and stores them as one 8-byte piece of bf16.  Grid (M / 128, Np / 64).
__global__ __launch_bounds__(256) void pointwise16_bwd_data_kernel(const StlDetPointwise16Bwd p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4;
    const int nsteps = p.Kp >> 5;
    int64_t row[2], base[2];
    bool ok[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        row[h] = (int64_t)blockIdx.x * 128 + wv * 32 + h * 16 + (lane & 15);
        ok[h] = row[h] < p.M;
        base[h] = ok[h] ? dy_row16(p, row[h]) : 0;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const V16* wp = reinterpret_cast<const V16*>(p.wt) + (int64_t)blockIdx.y * 4 * nsteps * 64 + lane;
    for (int ns = 0; ns < nsteps; ++ns) {
        const int n = ns * 32 + g * 8;
        V16 a[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) a[h] = ok[h] ? load_dy8(p, base[h], n) : zero16();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const V16 bw = wp[((int64_t)j * nsteps + ns) * 64];
#pragma unroll
            for (int h = 0; h < 2; ++h) mma16<__bf16>(acc[h][j], bw, a[h]);
        }
    }
    __bf16* dx = reinterpret_cast<__bf16*>(p.dx);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!ok[h]) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = blockIdx.y * 64 + j * 16 + g * 4;
            if (k >= p.Ci) continue;   // Ci % 8 == 0: the 4 channels are inside and 8-byte aligned
            uint2 ov;
            ov.x = pack2<__bf16>(acc[h][j][0], acc[h][j][1]), ov.y = pack2<__bf16>(acc[h][j][2], acc[h][j][3]);
            *reinterpret_cast<uint2*>(dx + row[h] * p.Ci + k) = ov;
        }
    }
}

constexpr int kW16Step = 64;                       // rows of M per LDS stage: two 32-deep MFMA steps
constexpr int kW16Ld = kW16Step / 2 + 4;           // dwords per LDS row: 64 rows of M as bf16 pairs, padded (144 bytes: 16-byte aligned)
constexpr int kSlab16Min = 256, kSlab16Max = 256;  // at least 256 rows per slab, at most 256 slabs

// Dword index of the 16-byte piece q (8 rows of M: 8 q .. 8 q + 7) of a staged column: the pieces of a column are swizzled by the
// column's group of 8, so that the 32 lanes of a dword write (8 column groups x 4 row pairs) meet 32 different banks.
__device__ __forceinline__ int w16_at(int col, int q) { return col * kW16Ld + ((q ^ ((col >> 3) & 7)) << 2); }

static inline int64_t slab_rows16(int64_t M) {
    const int64_t per = (M + kSlab16Max - 1) / kSlab16Max;
    const int64_t r = (per + kW16Step - 1) / kW16Step * kW16Step;
    return r < kSlab16Min ? kSlab16Min : r;
}

// dW'[k, n] = sum_m X[m, k] dY[m, n], db'[n] = sum_m dY[m, n] over one slab of rows.  The contraction runs over m, so both MFMA
// operands need 8 consecutive rows per lane: a workgroup stages 64 rows x 64 columns of X and of dY through LDS, transposed.  A
// thread loads 8 columns of two consecutive rows (16 bytes each; X converted from its 16-bit type to bf16, an fp32 dY rounded to
// bf16), pairs them in registers and writes 8 dwords (row m, row m + 1) to s[column][m / 2] (16-byte pieces swizzled, w16_at); a lane then reads its 8 rows of one
// column as 16 bytes.  Wave w owns k rows 16w .. 16w + 15 and 64 n columns (A = X^T: row = k, B = dY: column = n; D: row k =
// 4 (lane >> 4) + r, column n = lane & 15).  Rows past the slab, k past Ci and n past Co are staged as zeros.  The k-tile-0
// workgroups also add db' from the staged (bf16) dY: each wave its 16 rows of every stage in row order, then the four waves in
// wave order.  partial[slab][Ci * Co + Co].  Grid (slabs, Ci tiles, Co tiles).
template <typename TX>
__global__ __launch_bounds__(256) void pointwise16_bwd_weight_kernel(const StlDetPointwise16Bwd p, int64_t rows) {
    __shared__ __attribute__((aligned(16))) uint32_t sx[64 * kW16Ld];   // [k][m pair]
    __shared__ __attribute__((aligned(16))) uint32_t sy[64 * kW16Ld];   // [n][m pair]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4;
    const int k0 = blockIdx.y * 64, n0 = blockIdx.z * 64;
    const int64_t mbeg = (int64_t)blockIdx.x * rows;
    const int64_t mend = mbeg + rows < p.M ? mbeg + rows : p.M;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f;
    const int cg = (tid & 7) * 8, mp = tid >> 3;   // staging: columns cg .. cg + 7 of rows 2 mp, 2 mp + 1
    const int wpos = (((mp >> 2) ^ (tid & 7)) << 2) | (mp & 3);   // w16_at(column, mp >> 2) + (mp & 3) without the row
    const TX* x = reinterpret_cast<const TX*>(p.x);
    for (int64_t ms = mbeg; ms < mend; ms += kW16Step) {
        float fx[2][8];
        V16 vy[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t row = ms + 2 * mp + q;
            const bool ok = row < mend;
            V16 vx = zero16();
            if (ok && k0 + cg < p.Ci) vx = ldg16(x + row * p.Ci + k0 + cg);   // Ci % 8 == 0: inside or outside as a whole
            unpack<TX>(vx, fx[q]);
            vy[q] = ok ? load_dy8(p, dy_row16(p, row), n0 + cg) : zero16();
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sx[(cg + i) * kW16Ld + wpos] = pack2<__bf16>(fx[0][i], fx[1][i]);
            const uint32_t lo = (vy[0].w[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu, hi = (vy[1].w[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
            sy[(cg + i) * kW16Ld + wpos] = lo | (hi << 16);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kW16Step / 32; ++s) {
            const V16 a = *reinterpret_cast<const V16*>(&sx[w16_at(wv * 16 + (lane & 15), s * 4 + g)]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const V16 b = *reinterpret_cast<const V16*>(&sy[w16_at(j * 16 + (lane & 15), s * 4 + g)]);
                mma16<__bf16>(acc[j], a, b);
            }
        }
        if (blockIdx.y == 0) {   // wave w adds rows 16 w .. 16 w + 15 of the stage for column `lane`: two 16-byte reads
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const V16 v = *reinterpret_cast<const V16*>(&sy[w16_at(lane, wv * 2 + q)]);
                float f[8];
                unpack<__bf16>(v, f);
#pragma unroll
                for (int i = 0; i < 8; ++i) bacc += f[i];
            }
        }
        __syncthreads();
    }
    if (blockIdx.y == 0) {   // the four waves' sums, added in wave order (the loop's last barrier freed sx)
        float* red = reinterpret_cast<float*>(sx);
        red[wv * 64 + lane] = bacc;
        __syncthreads();
        bacc = (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
    }
    float* part = p.partial + (int64_t)blockIdx.x * ((int64_t)p.Ci * p.Co + p.Co);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (n >= p.Co) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + wv * 16 + g * 4 + r;
            if (k < p.Ci) part[(int64_t)k * p.Co + n] = acc[j][r];
        }
    }
    if (blockIdx.y == 0 && tid < 64 && n0 + tid < p.Co) part[(int64_t)p.Ci * p.Co + n0 + tid] = bacc;
}

// The depthwise data gradient, 8 channels per thread: dy bf16, taps fp32, z in TZ (swish'(z) in fp32 from the stored z), dx bf16.
template <typename TZ>
__global__ __launch_bounds__(256) void dwconv16_bwd_data_kernel(const __bf16* __restrict__ dy, const float* __restrict__ w,
                                                                const TZ* __restrict__ z, __bf16* __restrict__ dx, int B, int H, int W,
                                                                int C) {
    const int C8 = C >> 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * H * W * C8) return;
    const int c0 = (int)(e % C8) * 8;
    const int64_t pix = e / C8;
    const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int oy = y + 1 - ky;
        if (oy < 0 || oy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ox = x + 1 - kx;
            if (ox < 0 || ox >= W) continue;
            float f[8], wf[8];
            unpack<__bf16>(ldg16(dy + (((int64_t)b * H + oy) * W + ox) * C + c0), f);
            const float* wp = w + (ky * 3 + kx) * C + c0;
            unpack<float>(ldg16(wp), wf), unpack<float>(ldg16(wp + 4), wf + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += f[j] * wf[j];
        }
    }
    if (z) {
        float zf[8];
        unpack<TZ>(ldg16(z + pix * C + c0), zf);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] *= dswishf(zf[j]);
    }
    stg16(dx + pix * C + c0, pack<__bf16>(acc));
}

constexpr int kDw16PartMax = 512, kDw16PartPix = 256;   // at most 512 partial sums, at least 256 pixels each
static inline int dw16_bwd_parts(int64_t npix) {
    const int64_t p = (npix + kDw16PartPix - 1) / kDw16PartPix;
    return (int)(p < 1 ? 1 : (p > kDw16PartMax ? kDw16PartMax : p));
}

// partial[part][9][C]: a workgroup is 8 channel groups (64 channels) x 32 pixel lanes over the part's pixels; a thread adds its
// pixels in pixel order (fp32 products of x in TX and dy in bf16), then, tap by tap, one thread per channel adds the 32 lanes in
// lane order.
template <typename TX>
__global__ __launch_bounds__(256) void dwconv16_bwd_weight_kernel(const TX* __restrict__ x, const __bf16* __restrict__ dy,
                                                                  float* __restrict__ partial, int64_t npix, int H, int W, int C,
                                                                  int64_t per) {
    __shared__ float red[32][65];
    const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int c0 = (blockIdx.y * 8 + cl) * 8;
    const bool cok = c0 < C;   // C % 8 == 0: a group of 8 is inside or outside as a whole
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    float acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;
    if (cok) {
        for (int64_t p = p0 + pl; p < p1; p += 32) {
            const int px = (int)(p % W), py = (int)((p / W) % H);
            float gf[8];
            unpack<__bf16>(ldg16(dy + p * C + c0), gf);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = py - 1 + ky;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = px - 1 + kx;
                    if (ix < 0 || ix >= W) continue;
                    float xf[8];
                    unpack<TX>(ldg16(x + (p + (int64_t)(ky - 1) * W + (kx - 1)) * C + c0), xf);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[ky * 3 + kx][j] += xf[j] * gf[j];
                }
            }
        }
    }
    const int c = blockIdx.y * 64 + threadIdx.x;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[pl][cl * 8 + j] = acc[t][j];
        __syncthreads();
        if (threadIdx.x < 64 && c < C) {
            float a = 0.f;
            for (int q = 0; q < 32; ++q) a += red[q][threadIdx.x];
            partial[((int64_t)blockIdx.x * 9 + t) * C + c] = a;
        }
        __syncthreads();
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_det_loss(const float* reg, const float* cls, const float* anchors, const float* gt, const int32_t* offsets, int B,
                            int A, int nc, float alpha, float gamma, float box_weight, int32_t* assign, float* per_image, float* losses,
                            float* dreg, float* dlogit, int32_t* npos, void* stream) {
    STL_CHECK(B >= 1 && A >= 1 && nc >= 1, "det_loss: B %d A %d nc %d", B, A, nc);
    STL_CHECK(B <= 65535 && (int64_t)B * A * nc < (1ll << 31), "det_loss: B %d A %d nc %d too large", B, A, nc);
    STL_CHECK(reg && cls && anchors && offsets && assign && per_image && losses && dreg && dlogit && npos, "det_loss: null pointer");
    STL_CHECK(gamma >= 1.f && alpha >= 0.f && alpha <= 1.f, "det_loss: alpha %g (0 .. 1) gamma %g (>= 1)", (double)alpha, (double)gamma);
    STL_CHECK((((uintptr_t)reg | (uintptr_t)anchors | (uintptr_t)dreg) & 15) == 0, "det_loss: reg, anchors and dreg must be 16-byte aligned");
    STL_LAUNCH(det_loss_kernel, dim3(B), dim3(kLossThreads), 0, ST, reg, cls, anchors, gt, offsets, B, A, nc, alpha, gamma, box_weight,
               assign, per_image, dreg, dlogit, npos);
    STL_LAUNCH_CHECK("det_loss");
    STL_LAUNCH(det_loss_finish_kernel, dim3(1), dim3(64), 0, ST, (const float*)per_image, B, box_weight, losses);
    STL_LAUNCH_CHECK("det_loss_finish");
    return 0;
}

static int pointwise_bwd_check(const StlDetPointwiseBwd* p, const char* name) {
    STL_CHECK(p && p->dy, "%s: null pointer", name);
    STL_CHECK(p->M >= 1 && p->HW >= 1 && p->Ci >= 1 && p->Co >= 1, "%s: M %lld HW %d Ci %d Co %d", name, (long long)p->M, p->HW, p->Ci,
              p->Co);
    STL_CHECK((p->M + kT - 1) / kT < (1ll << 31), "%s: M too large", name);
    return 0;
}

extern "C" int stl_det_pointwise_bwd_data(const StlDetPointwiseBwd* p, void* stream) {
    if (pointwise_bwd_check(p, "det_pointwise_bwd_data")) return 1;
    STL_CHECK(p->w && p->dx, "det_pointwise_bwd_data: null pointer");
    STL_CHECK(p->Np % 64 == 0 && p->Np >= p->Co && p->Kp % 16 == 0 && p->Kp >= p->Ci, "det_pointwise_bwd_data: packed %d x %d for %d x %d",
              p->Kp, p->Np, p->Ci, p->Co);
    STL_CHECK(((uintptr_t)p->w & 15) == 0, "det_pointwise_bwd_data: w must be 16-byte aligned");
    STL_LAUNCH(pointwise_bwd_data_kernel, dim3((unsigned)((p->M + kT - 1) / kT), ceil_div(p->Ci, kT)), dim3(256), 0, ST, *p);
    STL_LAUNCH_CHECK("det_pointwise_bwd_data");
    return 0;
}

extern "C" int stl_det_pointwise_bwd_slabs(int64_t M) { return M >= 1 ? (int)((M + slab_rows(M) - 1) / slab_rows(M)) : 0; }

extern "C" int stl_det_pointwise_bwd_weight(const StlDetPointwiseBwd* p, void* stream) {
    if (pointwise_bwd_check(p, "det_pointwise_bwd_weight")) return 1;
    STL_CHECK(p->x && p->partial && p->dw && p->db, "det_pointwise_bwd_weight: null pointer");
    STL_CHECK(p->Ci <= 65535 * kT && p->Co <= 65535 * kT, "det_pointwise_bwd_weight: Ci %d Co %d", p->Ci, p->Co);
    const int64_t rows = slab_rows(p->M);
    const int slabs = stl_det_pointwise_bwd_slabs(p->M);
    STL_LAUNCH(pointwise_bwd_weight_kernel, dim3(slabs, ceil_div(p->Ci, kT), ceil_div(p->Co, kT)), dim3(256), 0, ST, *p, rows);
    STL_LAUNCH_CHECK("det_pointwise_bwd_weight");
    const int64_t n0 = (int64_t)p->Ci * p->Co, n = n0 + p->Co;
    STL_LAUNCH(sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float*)p->partial, slabs, n, n0, p->dw, p->db);
    STL_LAUNCH_CHECK("det_pointwise_bwd_weight_sum");
    return 0;
}

extern "C" int stl_det_dwconv_bwd_data(const float* dy, const float* w, const float* z, float* dx, int B, int H, int W, int C,
                                       void* stream) {
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1, "det_dwconv_bwd_data: B %d, %d x %d, C %d", B, H, W, C);
    STL_CHECK(dy && w && dx, "det_dwconv_bwd_data: null pointer");
    const int64_t n = (int64_t)B * H * W * C;
    STL_CHECK((n + 255) / 256 < (1ll << 31), "det_dwconv_bwd_data: too large");
    STL_LAUNCH(dwconv_bwd_data_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, dy, w, z, dx, B, H, W, C);
    STL_LAUNCH_CHECK("det_dwconv_bwd_data");
    return 0;
}

extern "C" int stl_det_dwconv_bwd_parts(int64_t npix) { return npix >= 1 ? dw_parts(npix) : 0; }

extern "C" int stl_det_dwconv_bwd_weight(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, int C,
                                         void* stream) {
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= 65535 * 64, "det_dwconv_bwd_weight: B %d, %d x %d, C %d", B, H, W, C);
    STL_CHECK(x && dy && partial && dw, "det_dwconv_bwd_weight: null pointer");
    const int64_t npix = (int64_t)B * H * W;
    const int parts = dw_parts(npix);
    const int64_t per = (npix + parts - 1) / parts;
    STL_LAUNCH(dwconv_bwd_weight_kernel, dim3(parts, ceil_div(C, 64)), dim3(256), 0, ST, x, dy, partial, npix, H, W, C, per);
    STL_LAUNCH_CHECK("det_dwconv_bwd_weight");
    const int64_t n = 9ll * C;
    STL_LAUNCH(sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float*)partial, parts, n, n, dw, dw);
    STL_LAUNCH_CHECK("det_dwconv_bwd_weight_sum");
    return 0;
}

// ------------------------------------------------------------------------------------------------ 16-bit entry points
// (al16, DET16_DTYPE and DET16_C8: common.cuh)

static int pointwise16_bwd_check(const StlDetPointwise16Bwd* p, const char* name) {
    STL_CHECK(p && p->dy, "%s: null pointer", name);
    STL_CHECK(p->M >= 1 && p->HW >= 1 && p->Co >= 1, "%s: M %lld HW %d Co %d", name, (long long)p->M, p->HW, p->Co);
    STL_CHECK(p->Ci >= 8 && p->Ci % 8 == 0, "%s: C %d (16-bit tensors need C %% 8 == 0)", name, p->Ci);
    STL_CHECK(p->dy_f32 == 0 || p->dy_f32 == 1, "%s: dy_f32 %d", name, p->dy_f32);
    STL_CHECK(p->dy_img_stride >= 0 && p->dy_row_stride >= p->Co && p->dy_off >= 0, "%s: dy strides %lld %lld offset %lld", name,
              (long long)p->dy_img_stride, (long long)p->dy_row_stride, (long long)p->dy_off);
    if (p->dy_f32) STL_CHECK(((uintptr_t)p->dy & 3) == 0, "%s: dy must be 4-byte aligned", name);
    else STL_CHECK(p->Co % 8 == 0 && p->dy_img_stride % 8 == 0 && p->dy_row_stride % 8 == 0 && p->dy_off % 8 == 0 && al16(p->dy),
                   "%s: a bf16 dy needs Co %d, strides and offset that are multiples of 8 and a 16-byte aligned pointer", name, p->Co);
    STL_CHECK((p->M + 127) / 128 < (1ll << 31), "%s: M too large", name);
    return 0;
}

extern "C" int stl_det_pointwise16_bwd_data(const StlDetPointwise16Bwd* p, void* stream) {
    if (pointwise16_bwd_check(p, "det_pointwise16_bwd_data")) return 1;
    STL_CHECK(p->wt && p->dx, "det_pointwise16_bwd_data: null pointer");
    STL_CHECK(p->Np % 64 == 0 && p->Np >= p->Ci && p->Kp % 32 == 0 && p->Kp >= p->Co,
              "det_pointwise16_bwd_data: transposed pack %d x %d for %d x %d", p->Kp, p->Np, p->Co, p->Ci);
    STL_CHECK(al16(p->wt) && al16(p->dx), "det_pointwise16_bwd_data: wt and dx must be 16-byte aligned");
    STL_LAUNCH(pointwise16_bwd_data_kernel, dim3((unsigned)((p->M + 127) / 128), p->Np / 64), dim3(256), 0, ST, *p);
    STL_LAUNCH_CHECK("det_pointwise16_bwd_data");
    return 0;
}

extern "C" int stl_det_pointwise16_bwd_slabs(int64_t M) { return M >= 1 ? (int)((M + slab_rows16(M) - 1) / slab_rows16(M)) : 0; }

extern "C" int stl_det_pointwise16_bwd_weight(const StlDetPointwise16Bwd* p, void* stream) {
    if (pointwise16_bwd_check(p, "det_pointwise16_bwd_weight")) return 1;
    DET16_DTYPE("det_pointwise16_bwd_weight", p->xdtype);
    STL_CHECK(p->x && p->partial && p->dw && p->db, "det_pointwise16_bwd_weight: null pointer");
    STL_CHECK(al16(p->x), "det_pointwise16_bwd_weight: x must be 16-byte aligned");
    STL_CHECK(p->Ci <= 65535 * 64 && p->Co <= 65535 * 64, "det_pointwise16_bwd_weight: Ci %d Co %d", p->Ci, p->Co);
    const int64_t rows = slab_rows16(p->M);
    const int slabs = stl_det_pointwise16_bwd_slabs(p->M);
    const dim3 grid(slabs, ceil_div(p->Ci, 64), ceil_div(p->Co, 64));
    if (p->xdtype == STL_BF16) STL_LAUNCH(pointwise16_bwd_weight_kernel<__bf16>, grid, dim3(256), 0, ST, *p, rows);
    else STL_LAUNCH(pointwise16_bwd_weight_kernel<f16>, grid, dim3(256), 0, ST, *p, rows);
    STL_LAUNCH_CHECK("det_pointwise16_bwd_weight");
    const int64_t n0 = (int64_t)p->Ci * p->Co, n = n0 + p->Co;
    STL_LAUNCH(sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float*)p->partial, slabs, n, n0, p->dw, p->db);
    STL_LAUNCH_CHECK("det_pointwise16_bwd_weight_sum");
    return 0;
}

extern "C" int stl_det_dwconv16_bwd_data(const void* dy, const float* w, const void* z, void* dx, int B, int H, int W, int C, int zdtype,
                                         void* stream) {
    STL_CHECK(B >= 1 && H >= 1 && W >= 1, "det_dwconv16_bwd_data: B %d, %d x %d", B, H, W);
    DET16_C8("det_dwconv16_bwd_data", C);
    if (z) DET16_DTYPE("det_dwconv16_bwd_data", zdtype);
    STL_CHECK(dy && w && dx, "det_dwconv16_bwd_data: null pointer");
    STL_CHECK(al16(dy) && al16(w) && al16(z) && al16(dx), "det_dwconv16_bwd_data: dy, w, z and dx must be 16-byte aligned");
    const int64_t n = (int64_t)B * H * W * (C / 8);
    STL_CHECK((n + 255) / 256 < (1ll << 31), "det_dwconv16_bwd_data: too large");
    const dim3 grid((unsigned)((n + 255) / 256));
    if (zdtype == STL_BF16) STL_LAUNCH(dwconv16_bwd_data_kernel<__bf16>, grid, dim3(256), 0, ST, (const __bf16*)dy, w, (const __bf16*)z, (__bf16*)dx, B, H, W, C);
    else STL_LAUNCH(dwconv16_bwd_data_kernel<f16>, grid, dim3(256), 0, ST, (const __bf16*)dy, w, (const f16*)z, (__bf16*)dx, B, H, W, C);
    STL_LAUNCH_CHECK("det_dwconv16_bwd_data");
    return 0;
}

extern "C" int stl_det_dwconv16_bwd_parts(int64_t npix) { return npix >= 1 ? dw16_bwd_parts(npix) : 0; }

extern "C" int stl_det_dwconv16_bwd_weight(int xdtype, const void* x, const void* dy, float* partial, float* dw, int B, int H, int W, int C,
                                           void* stream) {
    DET16_DTYPE("det_dwconv16_bwd_weight", xdtype);
    STL_CHECK(B >= 1 && H >= 1 && W >= 1, "det_dwconv16_bwd_weight: B %d, %d x %d", B, H, W);
    DET16_C8("det_dwconv16_bwd_weight", C);
    STL_CHECK(C <= 65535 * 64, "det_dwconv16_bwd_weight: C %d", C);
    STL_CHECK(x && dy && partial && dw, "det_dwconv16_bwd_weight: null pointer");
    STL_CHECK(al16(x) && al16(dy), "det_dwconv16_bwd_weight: x and dy must be 16-byte aligned");
    const int64_t npix = (int64_t)B * H * W;
    const int parts = dw16_bwd_parts(npix);
    const int64_t per = (npix + parts - 1) / parts;
    const dim3 grid(parts, ceil_div(C, 64));
    if (xdtype == STL_BF16) STL_LAUNCH(dwconv16_bwd_weight_kernel<__bf16>, grid, dim3(256), 0, ST, (const __bf16*)x, (const __bf16*)dy, partial, npix, H, W, C, per);
    else STL_LAUNCH(dwconv16_bwd_weight_kernel<f16>, grid, dim3(256), 0, ST, (const f16*)x, (const __bf16*)dy, partial, npix, H, W, C, per);
    STL_LAUNCH_CHECK("det_dwconv16_bwd_weight");
    const int64_t n = 9ll * C;
    STL_LAUNCH(sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float*)partial, parts, n, n, dw, dw);
    STL_LAUNCH_CHECK("det_dwconv16_bwd_weight_sum");
    return 0;
}
