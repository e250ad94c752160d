// AdaIN feed-forward stylisation on gfx950 (Huang & Belongie 2017; stlpose_amd/adain.py): the streaming kernels around the
// 3x3 convolutions, which are stl_conv_forward's, unchanged.
//
// stl_conv only knows zero padding and the network pads by reflection.  A reflection-padded 3x3 conv of an H x W map is the
// interior of a zero-padded "same" conv of the explicitly padded (H+2) x (W+2) map, so every layer is
//     stl_reflect_gather (writes the padded map) -> stl_conv_forward at (H+2) x (W+2) -> the next gather reads the interior.
// The ring of a conv's output is computed and never read.
//
//   stl_adain_input     NCHW fp32 image -> 3x3 patches taken by reflection, [B, H, W, 32]: conv1_1 as a 1x1 conv with K = 32
//   stl_reflect_gather  interior of the previous output -> padded input of the next conv, with the op between the two convs
//                       (copy / nearest x2 / 2x2 max-pool) and optionally the AdaIN affine fused in
//   stl_adain_stats     per (image, channel) mean, unbiased variance and sigma over the interior pixels, sums in fp64
//   stl_adain_affine    content and style statistics, style mix and alpha -> the one affine per (image, channel)
//   stl_adain_output    interior of the last conv's output, first 3 channels -> NCHW fp32, optionally clamped to [0, 1]
//
// All activation traffic is 16-byte vectors along the NHWC channel axis; element indices are 32-bit (checked by the launchers).
// fp contract is off for this file: the affine is a multiply and an add as written, so x * scale + offset in torch reproduces
// the gather bit for bit.
#include "common.cuh"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// torch's max: a NaN wins, else the larger value
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

template <typename T>
__global__ __launch_bounds__(256) void adain_input_kernel(const float* img, void* out, uint32_t total, int H, int W) {
    constexpr int KV = ET<T>::KV, VPP = 32 / KV;   // vectors per pixel
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < total; v += gridDim.x * 256u) {
        const uint32_t pi = v / VPP;
        const int part = (int)(v - pi * VPP);
        const int x = (int)(pi % (uint32_t)W);
        const uint32_t by = pi / (uint32_t)W;
        const int y = (int)(by % (uint32_t)H);
        const uint32_t b = by / (uint32_t)H;
        float f[KV];
#pragma unroll
        for (int j = 0; j < KV; ++j) {
            const int kk = part * KV + j;
            float val = 0.f;
            if (kk < 27) {
                const int tap = kk / 3, c = kk - tap * 3;
                const int iy = reflect1(y + tap / 3 - 1, H), ix = reflect1(x + tap % 3 - 1, W);
                val = img[((size_t)(b * 3 + c) * H + iy) * W + ix];
            }
            f[j] = val;
        }
        stg16((char*)out + (size_t)v * 16, pack<T>(f));
    }
}

// One workgroup per output row (b, y) of the padded map; its threads walk the row's (W + 2) * C / KV vectors.
// OP 0 copy, 1 nearest x2, 2 2x2 max-pool (floor); AFF: v * scale[b, c] + offset[b, c] on every value loaded.
// H, W: the interior size AFTER the op; Hs, Ws: the stored size of the source (its interior plus 2 * ring).
template <typename T, int OP, bool AFF>
__global__ __launch_bounds__(256) void reflect_gather_kernel(const void* src, void* out, int H, int W, int Hs, int Ws, int ring, int C,
                                                            const float* scale, const float* offset) {
    constexpr int KV = ET<T>::KV;
    const uint32_t VPC = (uint32_t)C / KV;
    const uint32_t row = blockIdx.x;
    const uint32_t b = row / (uint32_t)(H + 2);
    const int y = (int)(row - b * (uint32_t)(H + 2));
    const int iy = reflect1(y - 1, H);
    const uint32_t nvec = (uint32_t)(W + 2) * VPC;
    for (uint32_t i = threadIdx.x; i < nvec; i += 256u) {
        const uint32_t x = i / VPC;
        const int c0 = (int)(i - x * VPC) * KV;
        const int ix = reflect1((int)x - 1, W);
        int sy, sx;
        if (OP == 0) sy = iy, sx = ix;
        else if (OP == 1) sy = iy >> 1, sx = ix >> 1;
        else sy = 2 * iy, sx = 2 * ix;
        const uint32_t e = ((b * (uint32_t)Hs + (uint32_t)(sy + ring)) * (uint32_t)Ws + (uint32_t)(sx + ring)) * (uint32_t)C + (uint32_t)c0;
        const char* p = (const char*)src + (size_t)e * sizeof(T);
        V16 v = ldg16(p);
        if (OP == 2 || AFF) {
            float f[KV], sc[KV], of[KV];
            unpack<T>(v, f);
            if (AFF) {
#pragma unroll
                for (int j = 0; j < KV; j += 4) {
                    unpack<float>(ldg16(scale + (size_t)b * C + c0 + j), sc + j);
                    unpack<float>(ldg16(offset + (size_t)b * C + c0 + j), of + j);
                }
#pragma unroll
                for (int j = 0; j < KV; ++j) f[j] = f[j] * sc[j] + of[j];
            }
            if (OP == 2) {
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    float g[KV];
                    unpack<T>(ldg16(p + ((size_t)(k >> 1) * Ws + (k & 1)) * C * sizeof(T)), g);
#pragma unroll
                    for (int j = 0; j < KV; ++j) f[j] = max_nan(f[j], AFF ? g[j] * sc[j] + of[j] : g[j]);
                }
            }
            v = pack<T>(f);
        }
        stg16((char*)out + ((size_t)row * nvec + i) * 16, v);
    }
}

// Partial sums of one chunk of an image's interior pixels: thread t owns the KV channels of vector (t % VPC) and every
// (256 / VPC)-th pixel of the chunk; sum and sum of squares in fp64 (post-ReLU channels have mean >> sigma: fp32 sums of squares
// cancel).  The threads of one channel vector are added in a fixed order through LDS: partial[b][chunk][0 / 1][c], deterministic.
template <typename T>
__global__ __launch_bounds__(256) void adain_stats_kernel(const void* x, int H, int W, int ring, int C, int nchunk, double* partial) {
    constexpr int KV = ET<T>::KV;
    extern __shared__ __attribute__((aligned(16))) double red[];   // [group][2][C]
    const int VPC = C / KV, groups = 256 / VPC;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int g = threadIdx.x / VPC, cv = threadIdx.x - g * VPC;
    const int n = H * W, per = (n + nchunk - 1) / nchunk;
    const int p0 = chunk * per, p1 = min(n, p0 + per);
    const int Ws = W + 2 * ring, Hs = H + 2 * ring;
    double s1[KV], s2[KV];
#pragma unroll
    for (int j = 0; j < KV; ++j) s1[j] = 0.0, s2[j] = 0.0;
    if (g < groups) {
        for (int p = p0 + g; p < p1; p += groups) {
            const int py = p / W, px = p - py * W;
            const uint32_t e = (((uint32_t)b * Hs + (uint32_t)(py + ring)) * Ws + (uint32_t)(px + ring)) * (uint32_t)C + (uint32_t)(cv * KV);
            float f[KV];
            unpack<T>(ldg16((const char*)x + (size_t)e * sizeof(T)), f);
#pragma unroll
            for (int j = 0; j < KV; ++j) {
                const double d = (double)f[j];
                s1[j] += d;
                s2[j] = fma(d, d, s2[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < KV; ++j) {
            red[(size_t)(g * 2 + 0) * C + cv * KV + j] = s1[j];
            red[(size_t)(g * 2 + 1) * C + cv * KV + j] = s2[j];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        double a = 0.0;
        for (int k = 0; k < groups; ++k) a += red[(size_t)k * 2 * C + i];
        partial[((size_t)b * nchunk + chunk) * 2 * C + i] = a;
    }
}

// mean, unbiased variance and sigma = sqrt(var + eps) of one (image, channel) from its chunks, added in chunk order
__global__ __launch_bounds__(256) void adain_finish_kernel(const double* partial, int BC, int C, int nchunk, int n, double eps, float* mean,
                                                          float* var, float* sigma) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        s1 += partial[((size_t)b * nchunk + k) * 2 * C + c];
        s2 += partial[((size_t)b * nchunk + k) * 2 * C + C + c];
    }
    const double m = s1 / (double)n;
    double v = (s2 - s1 * m) / (double)(n - 1);
    if (v < 0.0) v = 0.0;
    mean[i] = (float)m;
    var[i] = (float)v;
    sigma[i] = (float)sqrt(v + eps);
}

// scale = alpha * s_s / s_c + (1 - alpha), offset = alpha * (m_s - m_c * s_s / s_c) with (m_s, s_s) = sum_k w[b, k] * style k's:
// AdaIN and the alpha blend as ONE affine of the content features.  fp64 inside, rounded once.
__global__ __launch_bounds__(256) void adain_affine_kernel(const float* mean_c, const float* var_c, const float* mean_s, const float* sigma_s,
                                                          const float* w, int BC, int C, int S, double alpha, double eps, float* scale,
                                                          float* offset) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    double ms = 0.0, ss = 0.0;
    for (int k = 0; k < S; ++k) {
        const double wk = (double)w[(size_t)b * S + k];
        ms += wk * (double)mean_s[(size_t)k * C + c];
        ss += wk * (double)sigma_s[(size_t)k * C + c];
    }
    const double r = ss / sqrt((double)var_c[i] + eps);
    scale[i] = (float)(alpha * r + (1.0 - alpha));
    offset[i] = (float)(alpha * (ms - (double)mean_c[i] * r));
}

template <typename T>
__global__ __launch_bounds__(256) void adain_output_kernel(const void* x, float* out, uint32_t total, int H, int W, int C, int clamp) {
    for (uint32_t pi = blockIdx.x * 256u + threadIdx.x; pi < total; pi += gridDim.x * 256u) {
        const int px = (int)(pi % (uint32_t)W);
        const uint32_t by = pi / (uint32_t)W;
        const int py = (int)(by % (uint32_t)H);
        const uint32_t b = by / (uint32_t)H;
        const uint32_t e = ((b * (uint32_t)(H + 2) + (uint32_t)(py + 1)) * (uint32_t)(W + 2) + (uint32_t)(px + 1)) * (uint32_t)C;
        float f[ET<T>::KV];
        unpack<T>(ldg16((const char*)x + (size_t)e * sizeof(T)), f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = f[c];
            if (clamp) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);   // (a NaN stays a NaN, as torch.clamp leaves it)
            out[((size_t)(b * 3 + c) * H + py) * W + px] = v;
        }
    }
}

inline int grid_for(size_t work, int cap) {
    size_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > (size_t)cap ? (size_t)cap : b));
}

}  // namespace

#define ST ((hipStream_t)stream)
#define ADAIN_DTYPE(name) STL_CHECK(dtype == STL_F32 || dtype == STL_BF16, name ": dtype %d (fp32 or bf16)", dtype)

extern "C" int stl_adain_input(int dtype, const float* img, void* out, int B, int H, int W, void* stream) {
    ADAIN_DTYPE("adain_input");
    STL_CHECK(img && out && B > 0 && H >= 2 && W >= 2, "adain_input: bad arguments (H, W >= 2 for the reflection)");
    const size_t total = (size_t)B * H * W * (dtype == STL_BF16 ? 4 : 8);
    STL_CHECK(total < (1ull << 31), "adain_input: %dx%dx%d is too large for 32-bit indices", B, H, W);
    if (dtype == STL_BF16)
        STL_LAUNCH(adain_input_kernel<__bf16>, dim3(grid_for(total, 4096)), dim3(256), 0, ST, img, out, (uint32_t)total, H, W);
    else
        STL_LAUNCH(adain_input_kernel<float>, dim3(grid_for(total, 4096)), dim3(256), 0, ST, img, out, (uint32_t)total, H, W);
    STL_LAUNCH_CHECK("adain_input");
    return 0;
}

extern "C" int stl_reflect_gather(int dtype, const void* src, void* out, int B, int Hs, int Ws, int ring, int C, int op, const float* scale,
                                  const float* offset, void* stream) {
    ADAIN_DTYPE("reflect_gather");
    STL_CHECK(src && out && B > 0 && Hs > 0 && Ws > 0 && (ring == 0 || ring == 1), "reflect_gather: bad arguments");
    STL_CHECK(op >= STL_GATHER_COPY && op <= STL_GATHER_POOL, "reflect_gather: op %d (0 copy, 1 up, 2 pool)", op);
    STL_CHECK(C > 0 && C % 8 == 0, "reflect_gather: C=%d must be a multiple of 8", C);
    STL_CHECK((scale == nullptr) == (offset == nullptr), "reflect_gather: scale and offset go together");
    const int H = op == STL_GATHER_UP ? 2 * Hs : (op == STL_GATHER_POOL ? Hs / 2 : Hs);
    const int W = op == STL_GATHER_UP ? 2 * Ws : (op == STL_GATHER_POOL ? Ws / 2 : Ws);
    STL_CHECK(H >= 2 && W >= 2, "reflect_gather: a %dx%d map has no reflection (2 pixels needed)", H, W);
    STL_CHECK((size_t)B * (Hs + 2 * ring) * (Ws + 2 * ring) * C < (1ull << 31) && (size_t)B * (H + 2) * (W + 2) * C < (1ull << 31),
              "reflect_gather: tensors of 2^31 or more elements are not supported (32-bit index arithmetic)");
    const dim3 grid((unsigned)(B * (H + 2)));
    const int Hst = Hs + 2 * ring, Wst = Ws + 2 * ring;
#define GATHER(TT, OP)                                                                                                             \
    do {                                                                                                                           \
        if (scale) STL_LAUNCH((reflect_gather_kernel<TT, OP, true>), grid, dim3(256), 0, ST, src, out, H, W, Hst, Wst, ring, C, scale, offset); \
        else STL_LAUNCH((reflect_gather_kernel<TT, OP, false>), grid, dim3(256), 0, ST, src, out, H, W, Hst, Wst, ring, C, scale, offset);      \
    } while (0)
#define GATHER_OP(TT)                                \
    do {                                             \
        if (op == STL_GATHER_COPY) GATHER(TT, 0);    \
        else if (op == STL_GATHER_UP) GATHER(TT, 1); \
        else GATHER(TT, 2);                          \
    } while (0)
    if (dtype == STL_BF16) GATHER_OP(__bf16);
    else GATHER_OP(float);
#undef GATHER_OP
#undef GATHER
    STL_LAUNCH_CHECK("reflect_gather");
    return 0;
}

extern "C" int stl_adain_stats(int dtype, const void* x, int B, int H, int W, int ring, int C, int nchunk, double* partial, float eps,
                               float* mean, float* var, float* sigma, void* stream) {
    ADAIN_DTYPE("adain_stats");
    STL_CHECK(x && partial && mean && var && sigma && B > 0 && (ring == 0 || ring == 1), "adain_stats: bad arguments");
    STL_CHECK(H > 0 && W > 0 && H * W >= 2, "adain_stats: the unbiased variance needs 2 pixels, got %dx%d", H, W);
    const int kv = dtype == STL_BF16 ? 8 : 4;
    STL_CHECK(C > 0 && C % 8 == 0 && C / kv <= 256, "adain_stats: C=%d must be a multiple of 8, at most %d", C, 256 * kv);
    STL_CHECK(nchunk >= 1 && nchunk <= 65535 && B <= 65535, "adain_stats: nchunk %d, B %d", nchunk, B);
    STL_CHECK((size_t)B * (H + 2 * ring) * (W + 2 * ring) * C < (1ull << 31), "adain_stats: tensors of 2^31 or more elements are not supported");
    const size_t lds = (size_t)(256 / (C / kv)) * 2 * C * sizeof(double);   // at most 256 * 2 * 8 * 8 = 32 KiB
    if (dtype == STL_BF16)
        STL_LAUNCH(adain_stats_kernel<__bf16>, dim3(nchunk, B), dim3(256), lds, ST, x, H, W, ring, C, nchunk, partial);
    else
        STL_LAUNCH(adain_stats_kernel<float>, dim3(nchunk, B), dim3(256), lds, ST, x, H, W, ring, C, nchunk, partial);
    STL_LAUNCH(adain_finish_kernel, dim3((B * C + 255) / 256), dim3(256), 0, ST, partial, B * C, C, nchunk, H * W, (double)eps, mean, var, sigma);
    STL_LAUNCH_CHECK("adain_stats");
    return 0;
}

extern "C" int stl_adain_affine(const float* mean_c, const float* var_c, const float* mean_s, const float* sigma_s, const float* weights, int B,
                                int C, int S, float alpha, float eps, float* scale, float* offset, void* stream) {
    STL_CHECK(mean_c && var_c && mean_s && sigma_s && weights && scale && offset && B > 0 && C > 0 && S > 0, "adain_affine: bad arguments");
    STL_CHECK(alpha >= 0.f && alpha <= 1.f, "adain_affine: alpha %g outside [0, 1]", (double)alpha);
    STL_LAUNCH(adain_affine_kernel, dim3((B * C + 255) / 256), dim3(256), 0, ST, mean_c, var_c, mean_s, sigma_s, weights, B * C, C, S,
               (double)alpha, (double)eps, scale, offset);
    STL_LAUNCH_CHECK("adain_affine");
    return 0;
}

extern "C" int stl_adain_output(int dtype, const void* x, float* out, int B, int H, int W, int C, int clamp, void* stream) {
    ADAIN_DTYPE("adain_output");
    STL_CHECK(x && out && B > 0 && H > 0 && W > 0, "adain_output: bad arguments");
    STL_CHECK(C >= 8 && C % 8 == 0, "adain_output: C=%d (the conv's padded Co, a multiple of 8)", C);
    STL_CHECK((size_t)B * (H + 2) * (W + 2) * C < (1ull << 31), "adain_output: tensors of 2^31 or more elements are not supported");
    const size_t total = (size_t)B * H * W;
    if (dtype == STL_BF16)
        STL_LAUNCH(adain_output_kernel<__bf16>, dim3(grid_for(total, 4096)), dim3(256), 0, ST, x, out, (uint32_t)total, H, W, C, clamp);
    else
        STL_LAUNCH(adain_output_kernel<float>, dim3(grid_for(total, 4096)), dim3(256), 0, ST, x, out, (uint32_t)total, H, W, C, clamp);
    STL_LAUNCH_CHECK("adain_output");
    return 0;
}
