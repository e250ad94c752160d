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
//   stl_det_pool_bwd   pool_bwd_kernel      the adjoint of a weightless pooled map (the first cell's t -> p6 -> p7): the pooled gather
//                                           with w^ = 1 and ds = dy, one thread per four channels of the input map (per channel
//                                           where C % 4 != 0); pool_gather is the one routine of both gathers
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

// The forward's scan of window (oy, ox) of the zero-padded 3x3 s2 max-pool of t, for V consecutive channels from c (V = 4: C % 4 == 0
// and t.x 16-byte aligned): the maximum m[k] and the winner's position (wy[k], wx[k]), the first strict maximum in (ky, kx) order;
// it lies outside the map when a padded tap (0 at its place) won.
template <int V>
__device__ __forceinline__ void pool_scan(const StlDetTerm& t, int b, int oy, int ox, int c, int C, float* m, int* wy, int* wx) {
    const int py = same_pad_before(t.H, 3, 2), px = same_pad_before(t.W, 3, 2);
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - py + ky;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - px + kx;
            float v[V];
            if (iy < 0 || iy >= t.H || ix < 0 || ix >= t.W) {
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = 0.f;
            } else {
                const float* src = t.x + (((int64_t)b * t.H + iy) * t.W + ix) * C + c;
                if constexpr (V == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(src);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) v[k] = src[k];
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (v[k] > m[k]) m[k] = v[k], wy[k] = iy, wx[k] = ix;
        }
    }
}

// fuse_read of detector.hip; for a pooled term also the winner's position (wy, wx), which lies outside the map when padding won
__device__ __forceinline__ float fuse_read_at(const StlDetTerm& t, int b, int y, int x, int c, int C, int& wy, int& wx) {
    if (t.mode == 0) return t.x[(((int64_t)b * t.H + y) * t.W + x) * C + c];
    if (t.mode == 1) return t.x[(((int64_t)b * t.H + (y >> 1)) * t.W + (x >> 1)) * C + c];
    float m;
    pool_scan<1>(t, b, y, x, c, C, &m, &wy, &wx);
    return m;
}

// The pooled gather of both backward kernels, for pixel (y, x) and V consecutive channels from c of the pooled map t (pooled into
// oH x oW): v[k] = the sum of scale * ds[window] over the up to four windows that hold the pixel, row-major, that the pixel won.
// Window oy holds rows 2 oy - py .. 2 oy - py + 2: oy in [ceil((y + py - 2) / 2), floor((y + py) / 2)], clipped to the output.
template <int V>
__device__ __forceinline__ void pool_gather(const StlDetTerm& t, int b, int y, int x, int c, int C, int oH, int oW,
                                            const float* __restrict__ ds, float scale, float* v) {
    const int py = same_pad_before(t.H, 3, 2), px = same_pad_before(t.W, 3, 2);
    const int oy0 = (y + py - 1) >> 1 > 0 ? (y + py - 1) >> 1 : 0, oy1 = (y + py) >> 1 < oH - 1 ? (y + py) >> 1 : oH - 1;
    const int ox0 = (x + px - 1) >> 1 > 0 ? (x + px - 1) >> 1 : 0, ox1 = (x + px) >> 1 < oW - 1 ? (x + px) >> 1 : oW - 1;
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            float m[V];
            int wy[V], wx[V];
#pragma unroll
            for (int k = 0; k < V; ++k) wy[k] = wx[k] = -1;
            pool_scan<V>(t, b, oy, ox, c, C, m, wy, wx);
            const float* d = ds + (((int64_t)b * oH + oy) * oW + ox) * C + c;
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(d);
                const float dv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (wy[k] == y && wx[k] == x) v[k] += scale * dv[k];
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (wy[k] == y && wx[k] == x) v[k] += scale * d[k];
            }
        }
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
    } else {
        pool_gather<1>(t, b, y, x, c, C, f.H, f.W, ds, wn[i], &v);
    }
    dx[e] = accumulate ? dx[e] + v : v;
}

// the weightless pooled node f (one mode-2 term): one thread per V consecutive channels of a pixel of the term's map
template <int V>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const StlDetFuse f, const float* __restrict__ dy, float* __restrict__ dx,
                                                       int accumulate) {
    const StlDetTerm& t = f.t[0];
    const int C = f.C, CV = C / V;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)f.B * t.H * t.W * CV) return;
    const int c = (int)(e % CV) * V;
    const int64_t pix = e / CV;
    const int x = (int)(pix % t.W), y = (int)((pix / t.W) % t.H), b = (int)(pix / ((int64_t)t.W * t.H));
    float v[V];
    pool_gather<V>(t, b, y, x, c, C, f.H, f.W, dy, 1.f, v);
    float* o = dx + pix * C + c;
    if constexpr (V == 4) {
        float4 q = make_float4(v[0], v[1], v[2], v[3]);
        if (accumulate) {
            const float4 a = *reinterpret_cast<const float4*>(o);
            q = make_float4(a.x + v[0], a.y + v[1], a.z + v[2], a.w + v[3]);
        }
        *reinterpret_cast<float4*>(o) = q;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = accumulate ? o[k] + v[k] : v[k];
    }
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

extern "C" int stl_det_pool_bwd(const StlDetFuse* f, const float* dy, float* dx, int accumulate, void* stream) {
    STL_CHECK(f && dy && dx, "det_pool_bwd: null pointer");
    STL_CHECK(f->B >= 1 && f->H >= 1 && f->W >= 1 && f->C >= 1, "det_pool_bwd: bad geometry");
    STL_CHECK(f->nterms == 1 && !f->wparam, "det_pool_bwd: %d terms%s (a weighted node is stl_det_fuse_bwd's)", f->nterms,
              f->wparam ? ", weights" : "");
    const StlDetTerm& t = f->t[0];
    STL_CHECK(t.x, "det_pool_bwd: term null");
    STL_CHECK(t.mode == 2 && t.H >= 1 && t.W >= 1 && (t.H + 1) / 2 == f->H && (t.W + 1) / 2 == f->W,
              "det_pool_bwd: term mode %d of %d x %d into %d x %d", t.mode, t.H, t.W, f->H, f->W);
    const int64_t ny = (int64_t)f->B * f->H * f->W * f->C, nx = (int64_t)f->B * t.H * t.W * f->C;
    STL_CHECK((nx + 255) / 256 < (1ll << 31), "det_pool_bwd: too large");
    STL_CHECK((uintptr_t)dy + 4 * (uintptr_t)ny <= (uintptr_t)dx || (uintptr_t)dx + 4 * (uintptr_t)nx <= (uintptr_t)dy,
              "det_pool_bwd: dy and dx overlap");
    const bool vec = f->C % 4 == 0 && (((uintptr_t)t.x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0;
    if (vec) {
        STL_LAUNCH(pool_bwd_kernel<4>, dim3((unsigned)((nx / 4 + 255) / 256)), dim3(256), 0, ST, *f, dy, dx, accumulate);
    } else {
        STL_LAUNCH(pool_bwd_kernel<1>, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, ST, *f, dy, dx, accumulate);
    }
    STL_LAUNCH_CHECK("det_pool_bwd");
    return 0;
}

extern "C" int stl_det_grad_add(const float* a, const float* b, const float* sa, const float* sb, float* out, int64_t n, void* stream) {
    STL_CHECK(a && b && out && n >= 1 && (n + 255) / 256 < (1ll << 31), "det_grad_add: null pointer or bad size %lld", (long long)n);
    STL_LAUNCH(grad_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, a, b, sa, sb, out, n);
    STL_LAUNCH_CHECK("det_grad_add");
    return 0;
}
