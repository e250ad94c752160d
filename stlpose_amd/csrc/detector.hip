// EfficientDet person detector on gfx950, NHWC (src/models/EfficientDet.py and models/efficientdet_utils/*,
// models/efficientnet/{model,utils,utils_extra}.py): preprocess, the MBConv backbone, BiFPN and the shared heads, anchor decode and class-aware NMS.
//
//   stl_det_preprocess  normalise + aspect-aware bilinear resize + zero canvas (efficientdet_utils/utils.py:190-239)
//   stl_det_stem        3 -> C 3x3/s2 same-padded conv, folded BN, swish (efficientnet/model.py:151-153)
//   stl_det_dwconv      depthwise kxk/s same-padded conv, folded BN bias, optional swish (MBConvBlock, SeparableConvBlock)
//   stl_det_se          squeeze-excitation scale[B, C] (efficientnet/model.py:84-89)
//   stl_det_pointwise   1x1 conv as a GEMM on v_mfma_f32_16x16x4_f32: SE scale on load, bias, swish / sigmoid, residual,
//                       strided output (the head headers write straight into the concatenated [B, A, k] outputs)
//   stl_det_pointwise_train  the same launch with swish, also keeping its pre-activation z (the heads' training forward,
//                       stlpose_amd/detector_train.py; the backward kernels are in detector_train.hip)
//   stl_det_fuse        BiFPN node swish(sum w_i * in_i) with same / nearest-2x / zero-padded 3x3 s2 max-pool inputs, the
//                       fast-attention weights normalised on the device (efficientdet_utils/model.py:163-233)
//   stl_det_decode      per-anchor class max, strict threshold, BBoxTransform, ClipBoxes, compaction in anchor order
//   stl_det_nms         torchvision.ops.batched_nms (0.4: class offsets, then nms) over any number of candidates
//
// The 16-bit compute modes (EfficientDetBackbone(compute_dtype="bf16" | "f16")) have entry points of their own; activations
// are stored as STL_BF16 / STL_F16 with C % 8 == 0 (8 channels per 16-byte access, any other C is an error), sums are fp32:
//
//   stl_det_stem16       fp32 canvas in, 16-bit out
//   stl_det_dwconv16     8 channels per thread; on request also the squeeze-excitation pooling sums, one slot per workgroup
//                        of pixels, taken from the fp32 values before rounding (a 16-bit plan has no pooling pass)
//   stl_det_se16         stl_det_se from those sums, added in slot order
//   stl_det_pointwise16  the GEMM on v_mfma_f32_16x16x32_{bf16,f16}, operands straight from global memory (no LDS): an NHWC
//                        row is the operand layout, the weights are packed to one 16-byte load per lane; 16-bit or strided fp32 output
//   stl_det_pointwise16_train  the same launch with swish and a 16-bit output, also keeping its pre-activation z rounded once to
//                        the 16-bit type (the 16-bit heads' training forward; the backward kernels are in detector_train.hip)
//   stl_det_fuse16       the BiFPN node on 16-bit tensors, attention weights fp32
//
// f16 activations past 65504 become inf; the model checks its head outputs (FloatingPointError) and points to bf16.  On the
// MI355X the 16-bit forwards take 5.2 ms (D0) and 11.7 ms (D3) at batch 32 against 14.3 and 34.2 ms in fp32
// (profiles/detector_bench.json).
//
// Every reduction runs in a fixed order (no float atomics): two runs give bitwise equal results.
#include "common.cuh"

namespace {

__device__ __forceinline__ float swishf(float x) { return x * (1.f / (1.f + __expf(-x))); }
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// TensorFlow "same" padding before the first row / column: extra = (ceil(n / s) - 1) * s - n + k, before = extra / 2
__host__ __device__ __forceinline__ int same_pad_before(int n, int k, int s) {
    const int extra = ((n + s - 1) / s - 1) * s - n + k;
    return (extra > 0 ? extra : 0) / 2;
}

// ------------------------------------------------------------------------------------------------ preprocess
// cv2.resize(INTER_LINEAR) on float32: src = (dst + 0.5) * scale - 0.5 in double, rounded to float, floor; a negative
// source index takes the first pixel with weight 1, one at or past the last takes the last pixel with weight 1.
struct LinTap {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ LinTap lin_tap(int d, double scale, int n) {
    const float f = (float)(((double)d + 0.5) * scale - 0.5);
    int i = (int)floorf(f);
    float a = f - (float)i;
    if (i < 0) i = 0, a = 0.f;
    if (i >= n - 1) i = n - 1, a = 0.f;
    LinTap t;
    t.i0 = i;
    t.i1 = min(i + 1, n - 1);
    t.w0 = 1.f - a;
    t.w1 = a;
    return t;
}

__global__ __launch_bounds__(256) void preprocess_kernel(const StlDetImage* __restrict__ imgs, int S, float* __restrict__ out) {
    const StlDetImage m = imgs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S * S) return;
    const int y = p / S, x = p - y * S;
    float* o = out + ((size_t)blockIdx.y * S * S + p) * 3;
    const float mean[3] = {0.406f, 0.456f, 0.485f}, istd[3] = {0.225f, 0.224f, 0.229f};
    if (y >= m.new_h || x >= m.new_w) {
        o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const bool same = m.new_h == m.old_h && m.new_w == m.old_w;
    LinTap ty, tx;
    if (same) {
        ty = LinTap{y, y, 1.f, 0.f};
        tx = LinTap{x, x, 1.f, 0.f};
    } else {
        ty = lin_tap(y, m.scale_y, m.old_h);
        tx = lin_tap(x, m.scale_x, m.old_w);
    }
    const int64_t plane = (int64_t)m.old_h * m.old_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[4];
        const int ys[2] = {ty.i0, ty.i1}, xs[2] = {tx.i0, tx.i1};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t e = (int64_t)ys[q >> 1] * m.old_w + xs[q & 1];
            const float raw = m.kind == 0 ? (float)reinterpret_cast<const uint8_t*>(m.src)[e * 3 + c] / 255.f
                                          : reinterpret_cast<const float*>(m.src)[c * plane + e];
            v[q] = (raw - mean[c]) / istd[c];   // transforms.Normalize: (x - mean) / std, then the resize
        }
        const float top = v[0] * tx.w0 + v[1] * tx.w1, bot = v[2] * tx.w0 + v[3] * tx.w1;
        o[c] = same ? v[0] : top * ty.w0 + bot * ty.w1;
    }
}

// ------------------------------------------------------------------------------------------------ stem and depthwise
// one thread per output (pixel, channel); w [3][3][3][Co], out NHWC, always BN-folded bias + swish
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ out, int B, int H, int W, int Ho, int Wo, int Co) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * Ho * Wo * Co) return;
    const int co = (int)(e % Co);
    const int64_t pix = e / Co;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
    const int py = same_pad_before(H, 3, 2), px = same_pad_before(W, 3, 2);
    float acc = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - py + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - px + kx;
            if (ix < 0 || ix >= W) continue;
            const float* xp = x + (((int64_t)b * H + iy) * W + ix) * 3;
            const float* wp = w + ((ky * 3 + kx) * 3) * Co + co;
            acc += xp[0] * wp[0] + xp[1] * wp[Co] + xp[2] * wp[2 * Co];
        }
    }
    out[e] = swishf(acc + bias[co]);
}

// one thread per output (pixel, channel); w [k][k][C]; bias null: none; act 1: swish
template <int K>
__global__ __launch_bounds__(256) void dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ out, int B, int H, int W, int C, int s, int Ho, int Wo, int act) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * Ho * Wo * C) return;
    const int c = (int)(e % C);
    const int64_t pix = e / C;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
    const int py = same_pad_before(H, K, s), px = same_pad_before(W, K, s);
    const int y0 = oy * s - py, x0 = ox * s - px;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int iy = y0 + ky;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int ix = x0 + kx;
            if (ix < 0 || ix >= W) continue;
            acc += x[(((int64_t)b * H + iy) * W + ix) * C + c] * w[(ky * K + kx) * C + c];
        }
    }
    if (bias) acc += bias[c];
    out[e] = act == 1 ? swishf(acc) : acc;
}

// ------------------------------------------------------------------------------------------------ squeeze-excitation
constexpr int kSeSplit = 32;   // pixel ranges per image of the pooling pass

// partial[b][split][c] = sum over the split's pixels, in pixel order
__global__ __launch_bounds__(256) void se_pool_kernel(const float* __restrict__ x, int HW, int C, float* __restrict__ partial) {
    const int b = blockIdx.y, sp = blockIdx.x;
    const int per = (HW + kSeSplit - 1) / kSeSplit;
    const int p0 = sp * per, p1 = min(HW, p0 + per);
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int p = p0; p < p1; ++p) acc += x[((int64_t)b * HW + p) * C + c];
        partial[((int64_t)b * kSeSplit + sp) * C + c] = acc;
    }
}

// one workgroup per image: mean -> reduce (w1 [Cs][C] + b1) -> swish -> expand (w2 [C][Cs] + b2) -> sigmoid
// partial [B][nparts][C], added in slot order
__global__ __launch_bounds__(256) void se_kernel(const float* __restrict__ partial, int nparts, int HW, int C, int Cs, const float* __restrict__ w1,
                                                 const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                 float* __restrict__ scale) {
    extern __shared__ float sm[];   // mean [C] | hidden [Cs]
    float* mean = sm;
    float* hid = sm + C;
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
#pragma unroll 8
        for (int sp = 0; sp < nparts; ++sp) acc += partial[((int64_t)b * nparts + sp) * C + c];
        mean[c] = acc / (float)HW;
    }
    __syncthreads();
    // one wave per hidden unit, lanes stride over C, then a fixed-order wave reduction
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j = wv; j < Cs; j += 4) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += w1[(int64_t)j * C + c] * mean[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) hid[j] = swishf(acc + b1[j]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = b2[c];
        for (int j = 0; j < Cs; ++j) acc += w2[(int64_t)c * Cs + j] * hid[j];
        scale[(int64_t)b * C + c] = sigmoidf_(acc);
    }
}

// ------------------------------------------------------------------------------------------------ pointwise GEMM
// out[m, n] = act(sum_k x[m, k] * (scale[img(m), k]) * w[k, n] + bias[n]) (+ residual[m, n]), m over B * HW pixels.
// Workgroup tile 64 x 64, 4 waves, wave w owns rows 16w .. 16w + 15 and all 64 columns (4 accumulators of 16 x 16);
// K in steps of 16 through LDS.  w is packed [Kp][Np] with zero padding (Kp % 16 == 0, Np % 64 == 0): activations are read
// with bounds checks, never padded.  KEEPZ: the value before the activation also goes to z [M, Co] (one kernel, so that the
// training forward of the heads is the inference forward bit for bit).
constexpr int kPwM = 64, kPwN = 64, kPwK = 16;

template <bool KEEPZ>
__global__ __launch_bounds__(256) void pointwise_kernel(const StlDetPointwise p, float* __restrict__ z) {
    __shared__ float sa[kPwK][kPwM + 4];   // [k][m]
    __shared__ float sb[kPwK][kPwN];       // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * kPwM;
    const int n0 = blockIdx.y * kPwN;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A staging: thread -> (row am, 4 consecutive k at ak)
    const int am = tid >> 2, ak = (tid & 3) * 4;
    const int64_t arow = m0 + am;
    const bool arow_ok = arow < p.M;
    const int aimg = arow_ok ? (int)(arow / p.HW) : 0;
    const float* xrow = p.x + (arow_ok ? arow : 0) * (int64_t)p.Ci;
    const float* srow = p.in_scale ? p.in_scale + (int64_t)aimg * p.Ci : nullptr;
    for (int k0 = 0; k0 < p.Ci; k0 += kPwK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + ak + q;
            float v = 0.f;
            if (arow_ok && k < p.Ci) {
                v = xrow[k];
                if (srow) v *= srow[k];
            }
            sa[ak + q][am] = v;
        }
        {   // B: 16 x 64 floats, one float4 per thread
            const int bk = tid >> 4, bn = (tid & 15) * 4;
            const float4 wv4 = *reinterpret_cast<const float4*>(p.w + (int64_t)(k0 + bk) * p.Np + n0 + bn);
            sb[bk][bn] = wv4.x, sb[bk][bn + 1] = wv4.y, sb[bk][bn + 2] = wv4.z, sb[bk][bn + 3] = wv4.w;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kPwK; ks += 4) {
            // A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
            const float a = sa[ks + (lane >> 4)][wv * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bv = sb[ks + (lane >> 4)][j * 16 + (lane & 15)];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C/D: col = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (n >= p.Co) continue;
        const float bias = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + wv * 16 + (lane >> 4) * 4 + r;
            if (m >= p.M) continue;
            float v = acc[j][r] + bias;
            if (KEEPZ) z[m * p.Co + n] = v;
            if (p.act == 1) v = swishf(v);
            else if (p.act == 2) v = sigmoidf_(v);
            if (p.residual) v += p.residual[m * p.Co + n];
            const int64_t img = m / p.HW, pix = m - img * p.HW;
            p.out[img * p.out_img_stride + pix * p.out_row_stride + p.out_off + n] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ BiFPN node
__device__ __forceinline__ float fuse_read(const StlDetTerm& t, int b, int y, int x, int c, int C) {
    if (t.mode == 0) return t.x[(((int64_t)b * t.H + y) * t.W + x) * C + c];
    if (t.mode == 1) return t.x[(((int64_t)b * t.H + (y >> 1)) * t.W + (x >> 1)) * C + c];
    // zero-padded (F.pad) 3x3 s2 max-pool with TF same padding: padded taps read 0
    const int py = same_pad_before(t.H, 3, 2), px = same_pad_before(t.W, 3, 2);
    float m = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y * 2 - py + ky;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x * 2 - px + kx;
            const float v = (iy < 0 || iy >= t.H || ix < 0 || ix >= t.W) ? 0.f : t.x[(((int64_t)b * t.H + iy) * t.W + ix) * C + c];
            m = v > m ? v : m;
        }
    }
    return m;
}

__global__ __launch_bounds__(256) void fuse_kernel(const StlDetFuse f) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)f.B * f.H * f.W * f.C) return;
    const int c = (int)(e % f.C);
    const int64_t pix = e / f.C;
    const int x = (int)(pix % f.W), y = (int)((pix / f.W) % f.H), b = (int)(pix / ((int64_t)f.W * f.H));
    if (!f.wparam) {   // a plain pooled map (p5_to_p6, p6_to_p7)
        f.out[e] = fuse_read(f.t[0], b, y, x, c, f.C);
        return;
    }
    // fast attention: w = relu(p) / (sum relu(p) + 1e-4), sums left to right
    float w[3], s = 0.f;
    for (int i = 0; i < f.nterms; ++i) {
        w[i] = f.wparam[i] > 0.f ? f.wparam[i] : 0.f;
        s += w[i];
    }
    s += 1e-4f;
    float acc = 0.f;
    for (int i = 0; i < f.nterms; ++i) acc += (w[i] / s) * fuse_read(f.t[i], b, y, x, c, f.C);
    f.out[e] = swishf(acc);
}

// ------------------------------------------------------------------------------------------------ decode
constexpr int kDecThreads = 1024;

__device__ __forceinline__ int scan_block(int v, int* sw, int& total) {
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
    for (int k = 0; k < kDecThreads / 64; ++k) {
        const int s = sw[k];
        base += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// one workgroup per image; anchors [A][4] (y1, x1, y2, x2), reg [B][A][4] (dy, dx, dh, dw), cls [B][A][nc]
__global__ __launch_bounds__(kDecThreads) void decode_kernel(const float* __restrict__ reg, const float* __restrict__ cls,
                                                             const float* __restrict__ anchors, int A, int nc, float thr, float xmax,
                                                             float ymax, float* boxes, float* scores, int32_t* classes,
                                                             int32_t* index, int32_t* count) {
#pragma clang fp contract(off)
    __shared__ int sw[kDecThreads / 64];
    const int b = blockIdx.x;
    int base = 0;
    for (int a0 = 0; a0 < A; a0 += kDecThreads) {
        const int a = a0 + threadIdx.x;
        float best = -INFINITY;
        int bc = 0;
        bool pass = false;
        if (a < A) {
            const float* cp = cls + ((int64_t)b * A + a) * nc;
            for (int k = 0; k < nc; ++k) {
                const float v = cp[k];
                if (v > best || k == 0) best = v, bc = k;
            }
            pass = best > thr;
        }
        int tot;
        const int pos = base + scan_block(pass ? 1 : 0, sw, tot);
        if (pass) {
            const float4 an = reinterpret_cast<const float4*>(anchors)[a];
            const float4 r = reinterpret_cast<const float4*>(reg)[(int64_t)b * A + a];
            const float yca = (an.x + an.z) / 2.f, xca = (an.y + an.w) / 2.f;
            const float ha = an.z - an.x, wa = an.w - an.y;
            const float w = expf(r.w) * wa, h = expf(r.z) * ha;
            const float yc = r.x * ha + yca, xc = r.y * wa + xca;
            float x1 = xc - w / 2.f, y1 = yc - h / 2.f, x2 = xc + w / 2.f, y2 = yc + h / 2.f;
            x1 = x1 < 0.f ? 0.f : x1;
            y1 = y1 < 0.f ? 0.f : y1;
            x2 = x2 > xmax ? xmax : x2;
            y2 = y2 > ymax ? ymax : y2;
            const int64_t o = (int64_t)b * A + pos;
            reinterpret_cast<float4*>(boxes)[o] = make_float4(x1, y1, x2, y2);
            scores[o] = best;
            classes[o] = bc;
            index[o] = a;
        }
        base += tot;
    }
    if (threadIdx.x == 0) count[b] = base;
}

// ------------------------------------------------------------------------------------------------ NMS
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

// one workgroup: max coordinate over all candidate boxes, then sbox[p] = boxes[order[p]] + class * (max + 1)
__global__ __launch_bounds__(1024) void nms_prep_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ classes,
                                                        const int32_t* __restrict__ order, int n, float4* __restrict__ sbox) {
#pragma clang fp contract(off)
    __shared__ float sm[16];
    float m = -INFINITY;
    for (int e = threadIdx.x; e < n * 4; e += 1024) m = fmaxf(m, boxes[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    float mx = sm[0];
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, sm[k]);
    const float step = mx + 1.f;
    for (int p = threadIdx.x; p < n; p += 1024) {
        const int r = order[p];
        const float off = (float)classes[r] * step;
        const float4 bx = reinterpret_cast<const float4*>(boxes)[r];
        sbox[p] = make_float4(bx.x + off, bx.y + off, bx.z + off, bx.w + off);
    }
}

// mask[i][cb] bit t: iou(sbox[i], sbox[64 cb + t]) > thr for 64 cb + t > i.  Grid (column blocks, row blocks), 64 threads.
__global__ __launch_bounds__(64) void nms_mask_kernel(const float4* __restrict__ sbox, int n, int nblk, float thr,
                                                      unsigned long long* __restrict__ mask) {
    const int cb = blockIdx.x, rb = blockIdx.y;
    if (cb < rb) return;
    __shared__ float4 cols[64];
    const int c = cb * 64 + threadIdx.x;
    if (c < n) cols[threadIdx.x] = sbox[c];
    __syncthreads();
    const int i = rb * 64 + threadIdx.x;
    if (i >= n) return;
    const float4 bi = sbox[i];
    const int nc = min(64, n - cb * 64);
    unsigned long long bits = 0;
    for (int t = 0; t < nc; ++t)
        if (cb * 64 + t > i && iou_tv(bi, cols[t]) > thr) bits |= 1ull << t;
    mask[(int64_t)i * nblk + cb] = bits;
}

// one wave: the greedy sweep in score order; removed bits in LDS; keep[] gets the kept positions (into the sorted order)
__global__ __launch_bounds__(64) void nms_sweep_kernel(const unsigned long long* __restrict__ mask, const int32_t* __restrict__ order,
                                                       int n, int nblk, int32_t* __restrict__ keep, int32_t* __restrict__ count) {
    extern __shared__ unsigned long long removed[];
    const int lane = threadIdx.x;
    for (int k = lane; k < nblk; k += 64) removed[k] = 0ull;
    __syncthreads();
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const int blk = i >> 6;
        const bool dead = (removed[blk] >> (i & 63)) & 1ull;   // uniform
        __syncthreads();
        if (dead) continue;
        if (lane == 0) keep[kept] = order[i];
        ++kept;
        const unsigned long long* row = mask + (int64_t)i * nblk;
        for (int k = blk + lane; k < nblk; k += 64) removed[k] |= row[k];
        __syncthreads();
    }
    if (lane == 0) *count = kept;
}

// ================================================================================================ 16-bit compute modes
// T = __bf16 or f16.  Activations are stored in T, NHWC, with C % 8 == 0, so that one 16-byte access moves 8 channels of a
// pixel; every sum, every weight but the pointwise ones, every bias and the SE / attention arithmetic are fp32, and a value
// is rounded to T once, when it is stored.

// fp32 canvas [B, H, W, 3] -> T [B, Ho, Wo, Co]; one thread per (pixel, 8 channels)
template <typename T>
__global__ __launch_bounds__(256) void stem16_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     T* __restrict__ out, int B, int H, int W, int Ho, int Wo, int Co) {
    const int C8 = Co >> 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * Ho * Wo * C8) return;
    const int c0 = (int)(e % C8) * 8;
    const int64_t pix = e / C8;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
    const int py = same_pad_before(H, 3, 2), px = same_pad_before(W, 3, 2);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - py + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - px + kx;
            if (ix < 0 || ix >= W) continue;
            const float* xp = x + (((int64_t)b * H + iy) * W + ix) * 3;
            const float* wp = w + ((ky * 3 + kx) * 3) * Co + c0;
            float wa[8], wb[8], wc[8];
            unpack<float>(ldg16(wp), wa), unpack<float>(ldg16(wp + 4), wa + 4);
            unpack<float>(ldg16(wp + Co), wb), unpack<float>(ldg16(wp + Co + 4), wb + 4);
            unpack<float>(ldg16(wp + 2 * Co), wc), unpack<float>(ldg16(wp + 2 * Co + 4), wc + 4);
            const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += x0 * wa[j] + x1 * wb[j] + x2 * wc[j];
        }
    }
    float bv[8];
    unpack<float>(ldg16(bias + c0), bv), unpack<float>(ldg16(bias + c0 + 4), bv + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = swishf(acc[j] + bv[j]);
    stg16(out + pix * Co + c0, pack<T>(acc));
}

// Depthwise: a workgroup is 8 channel groups (64 channels) x 32 pixel lanes of one image and walks `iters` rows of 32 pixels,
// so a slab of 64 channels of a pixel is one 128-byte run.  POOL: the workgroup also writes partial[b][blockIdx.x][c], the
// sum of its fp32 outputs before rounding: each thread adds its pixels in pixel order, then one thread per channel adds the 32
// pixel lanes in lane order (lanes and iterations past the last pixel add nothing).  stl_det_se16 adds the slots in order.
constexpr int kDwCG = 8, kDwPL = 32, kDwMaxParts = 64;
static inline int dw16_iters(int HW) { return HW > kDwPL * kDwMaxParts ? ceil_div(HW, kDwPL * kDwMaxParts) : 1; }
static inline int dw16_parts(int HW) { return ceil_div(HW, kDwPL * dw16_iters(HW)); }

template <typename T, int K, bool POOL>
__global__ __launch_bounds__(256) void dwconv16_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       T* __restrict__ out, float* __restrict__ partial, int H, int W, int C, int s,
                                                       int Ho, int Wo, int act, int iters, int nparts) {
    __shared__ float red[POOL ? kDwPL : 1][kDwCG * 8 + 1];
    const int cl = threadIdx.x & (kDwCG - 1), pl = threadIdx.x / kDwCG;
    const int c0 = (blockIdx.y * kDwCG + cl) * 8;
    const int b = blockIdx.z;
    const bool cok = c0 < C;   // C % 8 == 0: a group of 8 is inside or outside as a whole
    const int py = same_pad_before(H, K, s), px = same_pad_before(W, K, s);
    const int HW = Ho * Wo;
    float bv[8], psum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = psum[j] = 0.f;
    if (cok && bias) unpack<float>(ldg16(bias + c0), bv), unpack<float>(ldg16(bias + c0 + 4), bv + 4);
    for (int it = 0; it < iters; ++it) {
        const int p = (blockIdx.x * iters + it) * kDwPL + pl;
        if (!cok || p >= HW) continue;
        const int oy = p / Wo, ox = p - oy * Wo;
        const int y0 = oy * s - py, x0 = ox * s - px;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = y0 + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int ix = x0 + kx;
                if (ix < 0 || ix >= W) continue;
                float f[8], wf[8];
                unpack<T>(ldg16(x + (((int64_t)b * H + iy) * W + ix) * C + c0), f);
                const float* wp = w + (ky * K + kx) * C + c0;
                unpack<float>(ldg16(wp), wf), unpack<float>(ldg16(wp + 4), wf + 4);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += f[j] * wf[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[j] += bv[j];
            if (act == 1) acc[j] = swishf(acc[j]);
            if (POOL) psum[j] += acc[j];
        }
        stg16(out + ((int64_t)b * HW + p) * C + c0, pack<T>(acc));
    }
    if constexpr (POOL) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[pl][cl * 8 + j] = psum[j];
        __syncthreads();
        const int c = blockIdx.y * kDwCG * 8 + threadIdx.x;
        if (threadIdx.x < kDwCG * 8 && c < C) {
            float a = 0.f;
            for (int q = 0; q < kDwPL; ++q) a += red[q][threadIdx.x];
            partial[((int64_t)b * nparts + blockIdx.x) * C + c] = a;
        }
    }
}

// Pointwise GEMM on v_mfma_f32_16x16x32_{bf16,f16}, no LDS.  The weights are the MFMA's A operand and the pixels its B operand,
// so a lane ends up with 4 consecutive output channels of one pixel (D: row = 4 * (lane >> 4) + r is the channel, col =
// lane & 15 the pixel) and stores them as one 8-byte (T) or 16-byte-wide (fp32) piece of an NHWC row.  An NHWC row is already
// the operand layout: lane l loads the 8 channels k0 + 8 * (l >> 4) .. + 7 of pixel l & 15 in one 16-byte load (zero past M or
// Ci; Ci % 8 == 0, so a group of 8 never straddles the end of a row).  w is packed [Np / 16][Kp / 32][64 lanes][8]: one
// coalesced 16-byte load per lane and 16 x 32 tile, zero-padded to Kp % 32 == 0 and Np % 64 == 0.  A wave owns 32 pixels x 64
// channels (8 accumulators), a workgroup 128 pixels.
constexpr int kPw16M = 128, kPw16N = 64;

// KEEPZ (stl_det_pointwise16_train, 16-bit output only): also z[m, n] = the fp32 pre-activation rounded once to T.
template <typename T, bool F32OUT, bool KEEPZ = false>
__global__ __launch_bounds__(256) void pointwise16_kernel(const StlDetPointwise16 p, T* __restrict__ z) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4;
    const int ksteps = p.Kp >> 5;
    const T* x = reinterpret_cast<const T*>(p.x);
    int64_t row[2];
    bool ok[2];
    const T* xr[2];
    const float* sr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        row[h] = (int64_t)blockIdx.x * kPw16M + wv * 32 + h * 16 + (lane & 15);
        ok[h] = row[h] < p.M;
        xr[h] = x + (ok[h] ? row[h] : 0) * (int64_t)p.Ci;
        sr[h] = p.in_scale ? p.in_scale + (ok[h] ? row[h] / p.HW : 0) * (int64_t)p.Ci : nullptr;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const V16* wp = reinterpret_cast<const V16*>(p.w) + (int64_t)blockIdx.y * 4 * ksteps * 64 + lane;
    for (int ks = 0; ks < ksteps; ++ks) {
        const int k = ks * 32 + g * 8;
        V16 a[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            a[h] = zero16();
            if (ok[h] && k < p.Ci) {
                a[h] = ldg16(xr[h] + k);
                if (p.in_scale) {   // the SE scale: multiplied in fp32, rounded once to the operand type
                    float f[8], sc[8];
                    unpack<T>(a[h], f);
                    unpack<float>(ldg16(sr[h] + k), sc), unpack<float>(ldg16(sr[h] + k + 4), sc + 4);
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] *= sc[i];
                    a[h] = pack<T>(f);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const V16 bw = wp[((int64_t)j * ksteps + ks) * 64];
#pragma unroll
            for (int h = 0; h < 2; ++h) mma16<T>(acc[h][j], bw, a[h]);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!ok[h]) continue;
        const int64_t m = row[h];
        const int64_t img = m / p.HW, pix = m - img * p.HW;
        const int64_t obase = img * p.out_img_stride + pix * p.out_row_stride + p.out_off;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = blockIdx.y * kPw16N + j * 16 + g * 4;
            if (n >= p.Co) continue;
            float bv[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
            if (p.bias) unpack<float>(ldg16(p.bias + n), bv);   // bias is padded to Np
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[h][j][r] + bv[r];
            if constexpr (KEEPZ) {
                uint2 zv;
                zv.x = pack2<T>(v[0], v[1]), zv.y = pack2<T>(v[2], v[3]);
                *reinterpret_cast<uint2*>(z + m * p.Co + n) = zv;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (p.act == 1) v[r] = swishf(v[r]);
                else if (p.act == 2) v[r] = sigmoidf_(v[r]);
            }
            if constexpr (F32OUT) {   // any Co, any strides: element stores
                float* o = reinterpret_cast<float*>(p.out) + obase + n;
                const T* rs = reinterpret_cast<const T*>(p.residual) + m * p.Co + n;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r >= p.Co) break;
                    o[r] = p.residual ? v[r] + (float)rs[r] : v[r];
                }
            } else {   // Co % 4 == 0: the 4 channels are inside and 8-byte aligned
                if (p.residual) {
                    const uint2 rv = *reinterpret_cast<const uint2*>(reinterpret_cast<const T*>(p.residual) + m * p.Co + n);
                    float q[4];
                    unpack2<T>(rv.x, q[0], q[1]), unpack2<T>(rv.y, q[2], q[3]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += q[r];
                }
                uint2 ov;
                ov.x = pack2<T>(v[0], v[1]), ov.y = pack2<T>(v[2], v[3]);
                *reinterpret_cast<uint2*>(reinterpret_cast<T*>(p.out) + obase + n) = ov;
            }
        }
    }
}

// BiFPN node, 8 channels per thread
template <typename T>
__device__ __forceinline__ void fuse_read16(const StlDetTerm& t, int b, int y, int x, int c0, int C, float* f) {
    const T* src = reinterpret_cast<const T*>(t.x);
    if (t.mode == 0) return unpack<T>(ldg16(src + (((int64_t)b * t.H + y) * t.W + x) * C + c0), f);
    if (t.mode == 1) return unpack<T>(ldg16(src + (((int64_t)b * t.H + (y >> 1)) * t.W + (x >> 1)) * C + c0), f);
    const int py = same_pad_before(t.H, 3, 2), px = same_pad_before(t.W, 3, 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y * 2 - py + ky;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x * 2 - px + kx;
            float v[8];
            if (iy < 0 || iy >= t.H || ix < 0 || ix >= t.W) {   // padded taps read 0
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
            } else {
                unpack<T>(ldg16(src + (((int64_t)b * t.H + iy) * t.W + ix) * C + c0), v);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = v[j] > f[j] ? v[j] : f[j];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void fuse16_kernel(const StlDetFuse f) {
    const int C8 = f.C >> 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)f.B * f.H * f.W * C8) return;
    const int c0 = (int)(e % C8) * 8;
    const int64_t pix = e / C8;
    const int x = (int)(pix % f.W), y = (int)((pix / f.W) % f.H), b = (int)(pix / ((int64_t)f.W * f.H));
    T* o = reinterpret_cast<T*>(f.out) + pix * f.C + c0;
    float acc[8], v[8];
    if (!f.wparam) {
        fuse_read16<T>(f.t[0], b, y, x, c0, f.C, acc);
        stg16(o, pack<T>(acc));
        return;
    }
    float w[3], s = 0.f;
    for (int i = 0; i < f.nterms; ++i) {
        w[i] = f.wparam[i] > 0.f ? f.wparam[i] : 0.f;
        s += w[i];
    }
    s += 1e-4f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int i = 0; i < f.nterms; ++i) {
        fuse_read16<T>(f.t[i], b, y, x, c0, f.C, v);
        const float wi = w[i] / s;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += wi * v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = swishf(acc[j]);
    stg16(o, pack<T>(acc));
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_det_preprocess(const StlDetImage* imgs, int B, int S, float* out, void* stream) {
    STL_CHECK(B >= 0 && S >= 1 && S <= 4096, "det_preprocess: %d images, canvas %d", B, S);
    if (B == 0) return 0;
    STL_CHECK(imgs && out, "det_preprocess: null pointer");
    STL_LAUNCH(preprocess_kernel, dim3(ceil_div(S * S, 256), B), dim3(256), 0, ST, imgs, S, out);
    STL_LAUNCH_CHECK("det_preprocess");
    return 0;
}

extern "C" int stl_det_stem(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int Co, void* stream) {
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && Co >= 1, "det_stem: B %d, %d x %d, Co %d", B, H, W, Co);
    STL_CHECK(x && w && bias && out, "det_stem: null pointer");
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int64_t n = (int64_t)B * Ho * Wo * Co;
    STL_CHECK(n < (1ll << 31) * 256, "det_stem: too large");
    STL_LAUNCH(stem_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, x, w, bias, out, B, H, W, Ho, Wo, Co);
    STL_LAUNCH_CHECK("det_stem");
    return 0;
}

extern "C" int stl_det_dwconv(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C, int k, int s,
                              int act, void* stream) {
    STL_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1, "det_dwconv: B %d, %d x %d, C %d", B, H, W, C);
    STL_CHECK((k == 3 || k == 5) && (s == 1 || s == 2), "det_dwconv: k %d s %d (k in {3, 5}, s in {1, 2})", k, s);
    STL_CHECK(x && w && out, "det_dwconv: null pointer");
    const int Ho = (H + s - 1) / s, Wo = (W + s - 1) / s;
    const int64_t n = (int64_t)B * Ho * Wo * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (k == 3) STL_LAUNCH(dwconv_kernel<3>, grid, dim3(256), 0, ST, x, w, bias, out, B, H, W, C, s, Ho, Wo, act);
    else STL_LAUNCH(dwconv_kernel<5>, grid, dim3(256), 0, ST, x, w, bias, out, B, H, W, C, s, Ho, Wo, act);
    STL_LAUNCH_CHECK("det_dwconv");
    return 0;
}

extern "C" int stl_det_se(const float* x, int B, int HW, int C, int Cs, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* partial, float* scale, void* stream) {
    STL_CHECK(B >= 1 && HW >= 1 && C >= 1 && C <= 8192 && Cs >= 1 && Cs <= 1024, "det_se: B %d HW %d C %d Cs %d", B, HW, C, Cs);
    STL_CHECK(x && w1 && b1 && w2 && b2 && partial && scale, "det_se: null pointer");
    STL_LAUNCH(se_pool_kernel, dim3(kSeSplit, B), dim3(256), 0, ST, x, HW, C, partial);
    STL_LAUNCH_CHECK("det_se_pool");
    STL_LAUNCH(se_kernel, dim3(B), dim3(256), (size_t)(C + Cs) * 4, ST, (const float*)partial, kSeSplit, HW, C, Cs, w1, b1, w2, b2, scale);
    STL_LAUNCH_CHECK("det_se");
    return 0;
}

extern "C" int stl_det_se_workspace(int B) { return B * kSeSplit; }

static int pointwise_launch(const StlDetPointwise* p, float* z, hipStream_t st) {
    STL_CHECK(p && p->x && p->w && p->out, "det_pointwise: null pointer");
    STL_CHECK(p->M >= 1 && p->HW >= 1 && p->Ci >= 1 && p->Co >= 1, "det_pointwise: M %lld HW %d Ci %d Co %d", (long long)p->M, p->HW,
              p->Ci, p->Co);
    STL_CHECK(p->Np % kPwN == 0 && p->Np >= p->Co && p->Kp % kPwK == 0 && p->Kp >= p->Ci, "det_pointwise: packed %d x %d for %d x %d",
              p->Kp, p->Np, p->Ci, p->Co);
    STL_CHECK(p->act >= 0 && p->act <= 2, "det_pointwise: act %d", p->act);
    const int64_t mb = (p->M + kPwM - 1) / kPwM;
    STL_CHECK(mb < (1ll << 31), "det_pointwise: M too large");
    const dim3 grid((unsigned)mb, p->Np / kPwN);
    if (z) STL_LAUNCH(pointwise_kernel<true>, grid, dim3(256), 0, st, *p, z);
    else STL_LAUNCH(pointwise_kernel<false>, grid, dim3(256), 0, st, *p, z);
    STL_LAUNCH_CHECK("det_pointwise");
    return 0;
}

extern "C" int stl_det_pointwise(const StlDetPointwise* p, void* stream) { return pointwise_launch(p, nullptr, ST); }

extern "C" int stl_det_pointwise_train(const StlDetPointwise* p, float* z, void* stream) {
    STL_CHECK(z, "det_pointwise_train: null z");
    STL_CHECK(p && p->act == 1 && !p->residual, "det_pointwise_train: the layer must end in swish without a residual");
    return pointwise_launch(p, z, ST);
}

extern "C" int stl_det_fuse(const StlDetFuse* f, void* stream) {
    STL_CHECK(f && f->out && f->B >= 1 && f->H >= 1 && f->W >= 1 && f->C >= 1, "det_fuse: bad geometry");
    STL_CHECK(f->nterms >= 1 && f->nterms <= 3 && (f->wparam || f->nterms == 1), "det_fuse: %d terms", f->nterms);
    for (int i = 0; i < f->nterms; ++i) {
        const StlDetTerm& t = f->t[i];
        STL_CHECK(t.x, "det_fuse: term %d null", i);
        const bool ok = t.mode == 0 ? (t.H == f->H && t.W == f->W)
                      : t.mode == 1 ? (2 * t.H == f->H && 2 * t.W == f->W)
                      : t.mode == 2 ? ((t.H + 1) / 2 == f->H && (t.W + 1) / 2 == f->W) : false;
        STL_CHECK(ok, "det_fuse: term %d mode %d of %d x %d into %d x %d", i, t.mode, t.H, t.W, f->H, f->W);
    }
    const int64_t n = (int64_t)f->B * f->H * f->W * f->C;
    STL_LAUNCH(fuse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, *f);
    STL_LAUNCH_CHECK("det_fuse");
    return 0;
}

// ------------------------------------------------------------------------------------------------ 16-bit entry points
// (al16, DET16_DTYPE and DET16_C8 are in common.cuh, shared with detector_train.hip)

extern "C" int stl_det_stem16(int dtype, const float* x, const float* w, const float* bias, void* out, int B, int H, int W, int Co,
                              void* stream) {
    DET16_DTYPE("det_stem16", dtype);
    STL_CHECK(B >= 1 && H >= 1 && W >= 1, "det_stem16: B %d, %d x %d", B, H, W);
    DET16_C8("det_stem16", Co);
    STL_CHECK(x && w && bias && out, "det_stem16: null pointer");
    STL_CHECK(al16(w) && al16(bias) && al16(out), "det_stem16: w, bias and out must be 16-byte aligned");
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int64_t n = (int64_t)B * Ho * Wo * (Co / 8);
    STL_CHECK(n < (1ll << 31) * 256, "det_stem16: too large");
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == STL_BF16) STL_LAUNCH(stem16_kernel<__bf16>, grid, dim3(256), 0, ST, x, w, bias, (__bf16*)out, B, H, W, Ho, Wo, Co);
    else STL_LAUNCH(stem16_kernel<f16>, grid, dim3(256), 0, ST, x, w, bias, (f16*)out, B, H, W, Ho, Wo, Co);
    STL_LAUNCH_CHECK("det_stem16");
    return 0;
}

extern "C" int stl_det_dw16_parts(int HoWo) { return HoWo >= 1 ? dw16_parts(HoWo) : 0; }

template <typename T>
static int dwconv16_launch(const void* x, const float* w, const float* bias, void* out, float* partial, int B, int H, int W, int C, int k,
                           int s, int act, hipStream_t st) {
    const int Ho = (H + s - 1) / s, Wo = (W + s - 1) / s;
    const int iters = dw16_iters(Ho * Wo), nparts = dw16_parts(Ho * Wo);
    const dim3 grid(nparts, ceil_div(C / 8, kDwCG), B);
    const T* xi = (const T*)x;
    T* o = (T*)out;
    if (k == 3 && partial) STL_LAUNCH((dwconv16_kernel<T, 3, true>), grid, dim3(256), 0, st, xi, w, bias, o, partial, H, W, C, s, Ho, Wo, act, iters, nparts);
    else if (k == 3) STL_LAUNCH((dwconv16_kernel<T, 3, false>), grid, dim3(256), 0, st, xi, w, bias, o, partial, H, W, C, s, Ho, Wo, act, iters, nparts);
    else if (partial) STL_LAUNCH((dwconv16_kernel<T, 5, true>), grid, dim3(256), 0, st, xi, w, bias, o, partial, H, W, C, s, Ho, Wo, act, iters, nparts);
    else STL_LAUNCH((dwconv16_kernel<T, 5, false>), grid, dim3(256), 0, st, xi, w, bias, o, partial, H, W, C, s, Ho, Wo, act, iters, nparts);
    return 0;
}

extern "C" int stl_det_dwconv16(int dtype, const void* x, const float* w, const float* bias, void* out, float* partial, int B, int H,
                                int W, int C, int k, int s, int act, void* stream) {
    DET16_DTYPE("det_dwconv16", dtype);
    STL_CHECK(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "det_dwconv16: B %d, %d x %d", B, H, W);
    DET16_C8("det_dwconv16", C);
    STL_CHECK((k == 3 || k == 5) && (s == 1 || s == 2), "det_dwconv16: k %d s %d (k in {3, 5}, s in {1, 2})", k, s);
    STL_CHECK(x && w && out, "det_dwconv16: null pointer");
    STL_CHECK(al16(x) && al16(w) && al16(bias) && al16(out), "det_dwconv16: x, w, bias and out must be 16-byte aligned");
    STL_CHECK(C / 8 <= 65535 * kDwCG, "det_dwconv16: C %d", C);
    if (dtype == STL_BF16) dwconv16_launch<__bf16>(x, w, bias, out, partial, B, H, W, C, k, s, act, ST);
    else dwconv16_launch<f16>(x, w, bias, out, partial, B, H, W, C, k, s, act, ST);
    STL_LAUNCH_CHECK("det_dwconv16");
    return 0;
}

extern "C" int stl_det_se16(const float* partial, int B, int HW, int nparts, int C, int Cs, const float* w1, const float* b1,
                            const float* w2, const float* b2, float* scale, void* stream) {
    STL_CHECK(B >= 1 && HW >= 1 && nparts >= 1 && C >= 1 && C <= 8192 && Cs >= 1 && Cs <= 1024, "det_se16: B %d HW %d parts %d C %d Cs %d",
              B, HW, nparts, C, Cs);
    STL_CHECK(partial && w1 && b1 && w2 && b2 && scale, "det_se16: null pointer");
    STL_LAUNCH(se_kernel, dim3(B), dim3(256), (size_t)(C + Cs) * 4, ST, partial, nparts, HW, C, Cs, w1, b1, w2, b2, scale);
    STL_LAUNCH_CHECK("det_se16");
    return 0;
}

static int pointwise16_launch(const StlDetPointwise16* p, void* z, hipStream_t st) {
    STL_CHECK(p && p->x && p->w && p->out, "det_pointwise16: null pointer");
    DET16_DTYPE("det_pointwise16", p->dtype);
    STL_CHECK(p->M >= 1 && p->HW >= 1 && p->Co >= 1, "det_pointwise16: M %lld HW %d Co %d", (long long)p->M, p->HW, p->Co);
    STL_CHECK(p->Ci >= 8 && p->Ci % 8 == 0, "det_pointwise16: Ci %d (16-bit tensors need C %% 8 == 0)", p->Ci);
    STL_CHECK(p->Np % kPw16N == 0 && p->Np >= p->Co && p->Kp % 32 == 0 && p->Kp >= p->Ci, "det_pointwise16: packed %d x %d for %d x %d",
              p->Kp, p->Np, p->Ci, p->Co);
    STL_CHECK(p->act >= 0 && p->act <= 2, "det_pointwise16: act %d", p->act);
    STL_CHECK(al16(p->x) && al16(p->w) && al16(p->bias) && al16(p->in_scale), "det_pointwise16: x, w, bias and in_scale must be 16-byte aligned");
    if (!p->out_f32)   // 4 channels of a pixel are one 8-byte store
        STL_CHECK(p->Co % 4 == 0 && p->out_img_stride % 4 == 0 && p->out_row_stride % 4 == 0 && p->out_off % 4 == 0 && ((uintptr_t)p->out & 7) == 0 &&
                      ((uintptr_t)p->residual & 7) == 0,
                  "det_pointwise16: a 16-bit output needs Co %d, strides and offset that are multiples of 4 and 8-byte aligned pointers", p->Co);
    const int64_t mb = (p->M + kPw16M - 1) / kPw16M;
    STL_CHECK(mb < (1ll << 31), "det_pointwise16: M too large");
    const dim3 grid((unsigned)mb, p->Np / kPw16N);
    if (p->dtype == STL_BF16) {
        if (z) STL_LAUNCH((pointwise16_kernel<__bf16, false, true>), grid, dim3(256), 0, st, *p, (__bf16*)z);
        else if (p->out_f32) STL_LAUNCH((pointwise16_kernel<__bf16, true>), grid, dim3(256), 0, st, *p, (__bf16*)nullptr);
        else STL_LAUNCH((pointwise16_kernel<__bf16, false>), grid, dim3(256), 0, st, *p, (__bf16*)nullptr);
    } else {
        if (z) STL_LAUNCH((pointwise16_kernel<f16, false, true>), grid, dim3(256), 0, st, *p, (f16*)z);
        else if (p->out_f32) STL_LAUNCH((pointwise16_kernel<f16, true>), grid, dim3(256), 0, st, *p, (f16*)nullptr);
        else STL_LAUNCH((pointwise16_kernel<f16, false>), grid, dim3(256), 0, st, *p, (f16*)nullptr);
    }
    STL_LAUNCH_CHECK("det_pointwise16");
    return 0;
}

extern "C" int stl_det_pointwise16(const StlDetPointwise16* p, void* stream) { return pointwise16_launch(p, nullptr, ST); }

extern "C" int stl_det_pointwise16_train(const StlDetPointwise16* p, void* z, void* stream) {
    STL_CHECK(z && (((uintptr_t)z) & 7) == 0, "det_pointwise16_train: z null or not 8-byte aligned");
    STL_CHECK(p && p->act == 1 && !p->residual && !p->out_f32, "det_pointwise16_train: the layer must end in swish, without a residual, with a 16-bit output");
    return pointwise16_launch(p, z, ST);
}

extern "C" int stl_det_fuse16(const StlDetFuse* f, int dtype, void* stream) {
    DET16_DTYPE("det_fuse16", dtype);
    STL_CHECK(f && f->out && f->B >= 1 && f->H >= 1 && f->W >= 1, "det_fuse16: bad geometry");
    DET16_C8("det_fuse16", f->C);
    STL_CHECK(f->nterms >= 1 && f->nterms <= 3 && (f->wparam || f->nterms == 1), "det_fuse16: %d terms", f->nterms);
    STL_CHECK(al16(f->out), "det_fuse16: out must be 16-byte aligned");
    for (int i = 0; i < f->nterms; ++i) {
        const StlDetTerm& t = f->t[i];
        STL_CHECK(t.x && al16(t.x), "det_fuse16: term %d null or not 16-byte aligned", i);
        const bool ok = t.mode == 0 ? (t.H == f->H && t.W == f->W)
                      : t.mode == 1 ? (2 * t.H == f->H && 2 * t.W == f->W)
                      : t.mode == 2 ? ((t.H + 1) / 2 == f->H && (t.W + 1) / 2 == f->W) : false;
        STL_CHECK(ok, "det_fuse16: term %d mode %d of %d x %d into %d x %d", i, t.mode, t.H, t.W, f->H, f->W);
    }
    const int64_t n = (int64_t)f->B * f->H * f->W * (f->C / 8);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == STL_BF16) STL_LAUNCH(fuse16_kernel<__bf16>, grid, dim3(256), 0, ST, *f);
    else STL_LAUNCH(fuse16_kernel<f16>, grid, dim3(256), 0, ST, *f);
    STL_LAUNCH_CHECK("det_fuse16");
    return 0;
}

extern "C" int stl_det_decode(const float* reg, const float* cls, const float* anchors, int B, int A, int nc, float thr, float xmax,
                              float ymax, float* boxes, float* scores, int32_t* classes, int32_t* index, int32_t* count, void* stream) {
    STL_CHECK(B >= 0 && A >= 0 && nc >= 1, "det_decode: B %d A %d nc %d", B, A, nc);
    if (B == 0 || A == 0) return 0;
    STL_CHECK(reg && cls && anchors && boxes && scores && classes && index && count, "det_decode: null pointer");
    STL_LAUNCH(decode_kernel, dim3(B), dim3(kDecThreads), 0, ST, reg, cls, anchors, A, nc, thr, xmax, ymax, boxes, scores, classes,
               index, count);
    STL_LAUNCH_CHECK("det_decode");
    return 0;
}

extern "C" int64_t stl_det_nms_workspace(int n) {
    const int64_t nblk = (n + 63) / 64;
    return (int64_t)n * 16 + (int64_t)n * nblk * 8;
}

extern "C" int stl_det_nms(const float* boxes, const int32_t* classes, const int32_t* order, int n, double iou_thr, void* work,
                           int32_t* keep, int32_t* count, void* stream) {
    STL_CHECK(n >= 0 && n <= STL_DET_NMS_MAX, "det_nms: %d candidates (at most %d)", n, STL_DET_NMS_MAX);
    STL_CHECK(count, "det_nms: null count");
    if (n == 0) {
        (void)hipMemsetAsync(count, 0, 4, ST);
        return 0;
    }
    STL_CHECK(boxes && classes && order && work && keep, "det_nms: null pointer");
    const int nblk = (n + 63) / 64;
    // torchvision compares the float IoU with a double threshold: iou > t  <=>  iou > (the largest float <= t)
    float thr = (float)iou_thr;
    if ((double)thr > iou_thr) thr = nextafterf(thr, -INFINITY);
    float4* sbox = reinterpret_cast<float4*>(work);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(sbox + n);
    STL_LAUNCH(nms_prep_kernel, dim3(1), dim3(1024), 0, ST, boxes, classes, order, n, sbox);
    STL_LAUNCH_CHECK("det_nms_prep");
    STL_LAUNCH(nms_mask_kernel, dim3(nblk, nblk), dim3(64), 0, ST, (const float4*)sbox, n, nblk, thr, mask);
    STL_LAUNCH_CHECK("det_nms_mask");
    STL_LAUNCH(nms_sweep_kernel, dim3(1), dim3(64), (size_t)nblk * 8, ST, (const unsigned long long*)mask, order, n, nblk, keep, count);
    STL_LAUNCH_CHECK("det_nms_sweep");
    return 0;
}
