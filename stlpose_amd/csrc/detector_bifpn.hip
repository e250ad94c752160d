// Backward of the EfficientDet BiFPN node on gfx950 (stlpose_amd/detector_train.py, include/stlpose_hip_det_bifpn.h): the adjoint of
// fuse_kernel in detector.hip, out = swish(sum_i w^_i read_i) with same-size, nearest-2x and zero-padded 3x3 s2 max-pool terms.
// NHWC, fp32.  The forward keeps the node's output, not its pre-activation: s is recomputed here from the terms, with the forward's
// expression and order.
//
//   stl_det_fuse_bwd   fuse_bwd_ds_kernel   one thread per output element: s, ds = dy swish'(s), the mode-0 terms' dx = w^_i ds
//                                           (the same index), ds stored for the gathers, and per workgroup the fp64 partial sums
//                                           of dw^_i = sum ds read_i (a thread adds its elements in order, then an LDS tree)
//                      fuse_bwd_dw_kernel   the partial sums added in a fixed order by one workgroup, rounded once to fp32
//                      fuse_bwd_gather_kernel  one launch per requested term of mode 1 / 2, one thread per element of the TERM's map:
//                                           it gathers the ds of the outputs that read it (for a pooled term: of the windows it
//                                           won by the forward's scan), so nothing is scattered and there are no atomics
//   stl_det_grad_add   out = sa a + sb b, the scales read from the device (the two heads' gradients of a level, each times the
//                      gradient of its own loss)
//
// Every reduction runs in a fixed order (no float atomics): two runs give bitwise equal results.  Generic in C (64 for D0, 160 for D3).
#include "common.cuh"
#include "../../include/stlpose_hip_det_bifpn.h"

namespace {

// swish'(z) = s (1 + z (1 - s)), s = sigmoid(z): as in detector_train.hip
__device__ __forceinline__ float dswishf(float z) {
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
}

// TensorFlow "same" padding before the first row / column (detector.hip)
__host__ __device__ __forceinline__ int same_pad_before(int n, int k, int s) {
    const int extra = ((n + s - 1) / s - 1) * s - n + k;
    return (extra > 0 ? extra : 0) / 2;
}

// fuse_read of detector.hip; for a pooled term also the winner's position (wy, wx), which lies outside the map when padding won
__device__ __forceinline__ float fuse_read_at(const StlDetTerm& t, int b, int y, int x, int c, int C, int& wy, int& wx) {
    if (t.mode == 0) return t.x[(((int64_t)b * t.H + y) * t.W + x) * C + c];
    if (t.mode == 1) return t.x[(((int64_t)b * t.H + (y >> 1)) * t.W + (x >> 1)) * C + c];
    const int py = same_pad_before(t.H, 3, 2), px = same_pad_before(t.W, 3, 2);
    float m = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y * 2 - py + ky;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x * 2 - px + kx;
            const float v = (iy < 0 || iy >= t.H || ix < 0 || ix >= t.W) ? 0.f : t.x[(((int64_t)b * t.H + iy) * t.W + ix) * C + c];
            if (v > m) m = v, wy = iy, wx = ix;
        }
    }
    return m;
}

// the forward's normalised weights: w = relu(p) / (sum relu(p) + 1e-4), summed left to right
__device__ __forceinline__ void fuse_weights(const StlDetFuse& f, float* wn) {
    float w[3], s = 0.f;
    for (int i = 0; i < f.nterms; ++i) {
        w[i] = f.wparam[i] > 0.f ? f.wparam[i] : 0.f;
        s += w[i];
    }
    s += 1e-4f;
    for (int i = 0; i < f.nterms; ++i) wn[i] = w[i] / s;
}

constexpr int kDsBlocksMax = 1024;   // at most this many partial sums per term
static inline int ds_blocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > kDsBlocksMax ? kDsBlocksMax : b));
}

// elements [blockIdx.x * per, + per) of the output, per % 256 == 0; partial[block][3]
__global__ __launch_bounds__(256) void fuse_bwd_ds_kernel(const StlDetFuse f, const float* __restrict__ dy, const StlDetFuseBwd g,
                                                          float* __restrict__ ds, double* __restrict__ partial, int64_t per) {
    __shared__ double red[3][256];
    const int64_t n = (int64_t)f.B * f.H * f.W * f.C;
    const int64_t e0 = (int64_t)blockIdx.x * per, e1 = e0 + per < n ? e0 + per : n;
    float wn[3];
    fuse_weights(f, wn);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const int c = (int)(e % f.C);
        const int64_t pix = e / f.C;
        const int x = (int)(pix % f.W), y = (int)((pix / f.W) % f.H), b = (int)(pix / ((int64_t)f.W * f.H));
        float r[3], s = 0.f;
        int wy, wx;
        for (int i = 0; i < f.nterms; ++i) {
            r[i] = fuse_read_at(f.t[i], b, y, x, c, f.C, wy, wx);
            s += wn[i] * r[i];
        }
        const float d = dy[e] * dswishf(s);
        if (ds) ds[e] = d;
        for (int i = 0; i < f.nterms; ++i) {
            acc[i] += (double)d * (double)r[i];
            if (f.t[i].mode == 0 && g.dx[i]) {
                const float v = wn[i] * d;
                g.dx[i][e] = g.accumulate[i] ? g.dx[i][e] + v : v;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) red[i][threadIdx.x] = acc[i];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int i = 0; i < 3; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// dwhat[i] = sum over the nb partial sums: thread t adds partials t, t + 256, ... in order, then an LDS tree; one workgroup
__global__ __launch_bounds__(256) void fuse_bwd_dw_kernel(const double* __restrict__ partial, int nb, int nterms, float* __restrict__ dwhat) {
    __shared__ double red[3][256];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < nb; j += 256) {
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[i] += partial[(int64_t)j * 3 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) red[i][threadIdx.x] = acc[i];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int i = 0; i < 3; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + s];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nterms) dwhat[threadIdx.x] = (float)red[threadIdx.x][0];
}

// term i (mode 1 or 2): one thread per element of its own map
__global__ __launch_bounds__(256) void fuse_bwd_gather_kernel(const StlDetFuse f, int i, const float* __restrict__ ds,
                                                              float* __restrict__ dx, int accumulate) {
    const StlDetTerm& t = f.t[i];
    const int C = f.C;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)f.B * t.H * t.W * C) return;
    const int c = (int)(e % C);
    const int64_t pix = e / C;
    const int x = (int)(pix % t.W), y = (int)((pix / t.W) % t.H), b = (int)(pix / ((int64_t)t.W * t.H));
    float wn[3];
    fuse_weights(f, wn);
    float v;
    if (t.mode == 1) {   // read by outputs (2y .. 2y + 1, 2x .. 2x + 1), those inside H x W
        float sum = 0.f;
        for (int oy = 2 * y; oy <= 2 * y + 1 && oy < f.H; ++oy)
            for (int ox = 2 * x; ox <= 2 * x + 1 && ox < f.W; ++ox) sum += ds[(((int64_t)b * f.H + oy) * f.W + ox) * C + c];
        v = wn[i] * sum;
    } else {   // window oy holds rows 2 oy - py .. 2 oy - py + 2: oy in [ceil((y + py - 2) / 2), floor((y + py) / 2)], clipped to the output
        const int py = same_pad_before(t.H, 3, 2), px = same_pad_before(t.W, 3, 2);
        const int oy0 = (y + py - 1) >> 1 > 0 ? (y + py - 1) >> 1 : 0, oy1 = (y + py) >> 1 < f.H - 1 ? (y + py) >> 1 : f.H - 1;
        const int ox0 = (x + px - 1) >> 1 > 0 ? (x + px - 1) >> 1 : 0, ox1 = (x + px) >> 1 < f.W - 1 ? (x + px) >> 1 : f.W - 1;
        v = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                int wy = -1, wx = -1;
                fuse_read_at(t, b, oy, ox, c, C, wy, wx);
                if (wy == y && wx == x) v += wn[i] * ds[(((int64_t)b * f.H + oy) * f.W + ox) * C + c];
            }
    }
    dx[e] = accumulate ? dx[e] + v : v;
}

__global__ __launch_bounds__(256) void grad_add_kernel(const float* a, const float* b, const float* __restrict__ sa,
                                                       const float* __restrict__ sb, float* out, int64_t n) {   // out may be a or b
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float va = sa ? *sa * a[e] : a[e], vb = sb ? *sb * b[e] : b[e];
    out[e] = va + vb;
}

}  // namespace

#define ST ((hipStream_t)stream)

// floats: the partial sums (fp64, in front: the workspace is 8-byte aligned), then ds
extern "C" int64_t stl_det_fuse_bwd_workspace(int64_t n) { return n >= 1 ? n + 2 * 3 * (int64_t)kDsBlocksMax : 0; }

extern "C" int stl_det_fuse_bwd(const StlDetFuse* f, const float* dy, const StlDetFuseBwd* g, float* workspace, float* dwhat, void* stream) {
    STL_CHECK(f && g && dy && workspace && dwhat, "det_fuse_bwd: null pointer");
    STL_CHECK(f->B >= 1 && f->H >= 1 && f->W >= 1 && f->C >= 1, "det_fuse_bwd: bad geometry");
    STL_CHECK(f->nterms >= 1 && f->nterms <= 3 && f->wparam, "det_fuse_bwd: %d terms%s", f->nterms, f->wparam ? "" : ", no weights");
    STL_CHECK(((uintptr_t)workspace & 7) == 0, "det_fuse_bwd: the workspace must be 8-byte aligned");
    bool gather = false;
    for (int i = 0; i < f->nterms; ++i) {
        const StlDetTerm& t = f->t[i];
        STL_CHECK(t.x, "det_fuse_bwd: term %d null", i);
        const bool ok = t.mode == 0 ? (t.H == f->H && t.W == f->W)
                      : t.mode == 1 ? ((f->H + 1) / 2 == t.H && (f->W + 1) / 2 == t.W)
                      : t.mode == 2 ? ((t.H + 1) / 2 == f->H && (t.W + 1) / 2 == f->W) : false;
        STL_CHECK(ok, "det_fuse_bwd: term %d mode %d of %d x %d into %d x %d", i, t.mode, t.H, t.W, f->H, f->W);
        STL_CHECK(((int64_t)f->B * t.H * t.W * f->C + 255) / 256 < (1ll << 31), "det_fuse_bwd: term %d too large", i);
        gather = gather || (t.mode != 0 && g->dx[i]);
    }
    const int64_t n = (int64_t)f->B * f->H * f->W * f->C;
    const int nb = ds_blocks(n);
    const int64_t per = ((n + nb - 1) / nb + 255) / 256 * 256;
    double* partial = reinterpret_cast<double*>(workspace);
    float* ds = workspace + 2 * 3 * kDsBlocksMax;
    STL_LAUNCH(fuse_bwd_ds_kernel, dim3((unsigned)nb), dim3(256), 0, ST, *f, dy, *g, gather ? ds : (float*)nullptr, partial, per);
    STL_LAUNCH_CHECK("det_fuse_bwd");
    STL_LAUNCH(fuse_bwd_dw_kernel, dim3(1), dim3(256), 0, ST, (const double*)partial, nb, f->nterms, dwhat);
    STL_LAUNCH_CHECK("det_fuse_bwd");
    for (int i = 0; i < f->nterms; ++i) {
        const StlDetTerm& t = f->t[i];
        if (t.mode == 0 || !g->dx[i]) continue;
        const int64_t nt = (int64_t)f->B * t.H * t.W * f->C;
        STL_LAUNCH(fuse_bwd_gather_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, ST, *f, i, (const float*)ds, g->dx[i], g->accumulate[i]);
        STL_LAUNCH_CHECK("det_fuse_bwd");
    }
    return 0;
}

extern "C" int stl_det_grad_add(const float* a, const float* b, const float* sa, const float* sb, float* out, int64_t n, void* stream) {
    STL_CHECK(a && b && out && n >= 1 && (n + 255) / 256 < (1ll << 31), "det_grad_add: null pointer or bad size %lld", (long long)n);
    STL_LAUNCH(grad_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, a, b, sa, sb, out, n);
    STL_LAUNCH_CHECK("det_grad_add");
    return 0;
}
