// Detector training / validation batches on gfx950: what data/Detection_Dataset.py + ResizeImageDetection
// (data/custom_transforms.py:36-67) + `imgs / 255` + stl_det_preprocess do between an image's record and the network's canvas, as
// ONE launch per batch over images and annotation tables that stay on the device (stlpose_amd/det_data.py).  The C ABI and the
// definition of every value are in include/stlpose_hip_det_batch.h.
//
//   stl_det_batch   one thread per canvas pixel (grid.y = the image): the 12-byte stores of neighbouring threads coalesce, the byte
//                   gathers of the source image are the only irregular traffic.  Nothing between the source bytes and the canvas
//                   is stored: a canvas pixel taps up to 2 x 2 pixels of the S1 x S1 square, each of which is 0 (the padding, which
//                   Normalize turns into -mean / std) or the rounded blend of up to 2 x 2 source pixels.  The first workgroup of
//                   every image also sums the counts of the images before it (LDS, integers) and writes the image's rows of the
//                   ground-truth table.  No scratch.
//
// The kernel draws nothing: the flip draws come in as a table, so it is a pure function of its inputs.
//
// Exactness.  fp contract is off for this file: stage 1 and the boxes are the expressions of tests/det_batch_ref.py, operation for
// operation.  Stage 2 has to equal preprocess_kernel (detector.hip), whose unit is built with contraction on; the three places where
// the compiler fuses there -- the tap position and the two horizontal blends -- are written as explicit fma here, and
// tests/test_det_batch_gpu.py holds the two kernels to each other bit for bit.
#include "common.cuh"
#include "../../include/stlpose_hip_det_batch.h"

#pragma clang fp contract(off)

namespace {

struct Tap {
    int i0, i1;
    float w0, w1;
};

// lin_tap of detector.hip from the source position f: a negative index takes the first pixel with weight 1, one at or past the
// last takes the last pixel with weight 1
__device__ __forceinline__ Tap tap_at(float f, int n) {
    int i = (int)floorf(f);
    float a = f - (float)i;
    if (i < 0) i = 0, a = 0.f;
    if (i >= n - 1) i = n - 1, a = 0.f;
    return Tap{i, min(i + 1, n - 1), 1.f - a, a};
}

struct Geo {   // one image of the batch
    const uint8_t* img;
    int h, w, rh, rw, flip;
    double sy, sx;   // stage 1: old / new
    float scale;
    bool ok;
};

__device__ __forceinline__ Geo geometry(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int32_t* src_hw,
                                        const int64_t* index, int64_t N, const double* draws, int flip_enabled, int S1, int b) {
    Geo g;
    const int64_t row = index[b], off = src_off[b];
    g.h = src_hw[2 * b], g.w = src_hw[2 * b + 1];
    g.ok = row >= 0 && row < N && g.h >= 1 && g.w >= 1 && off >= 0 && off <= src_bytes &&
           (int64_t)g.h * g.w <= (src_bytes - off) / 3;
    g.img = src + (g.ok ? off : 0);
    g.flip = flip_enabled && draws != nullptr && draws[b] <= 0.5;
    g.rh = g.rw = 0, g.sy = g.sx = 1.0, g.scale = 0.f;
    if (!g.ok) return g;
    double scale;
    if (g.h > g.w) {   // ResizeImageDetection.__call__
        scale = (double)S1 / (double)g.h;
        g.rh = S1, g.rw = (int)((double)g.w * scale);
    } else {
        scale = (double)S1 / (double)g.w;
        g.rh = (int)((double)g.h * scale), g.rw = S1;
    }
    g.scale = (float)scale;
    if (g.rh >= 1 && g.rw >= 1) g.sy = 1.0 / ((double)g.rh / (double)g.h), g.sx = 1.0 / ((double)g.rw / (double)g.w);
    return g;
}

// The three levels (0 .. 255, as floats) of pixel (y, x) of the S1 x S1 stage-1 image.
__device__ __forceinline__ void stage1_pixel(const Geo& g, int y, int x, float* lvl) {
    if (y >= g.rh || x >= g.rw) {
        lvl[0] = lvl[1] = lvl[2] = 0.f;
        return;
    }
    const int xs = g.flip ? g.rw - 1 - x : x;
    const Tap ty = tap_at((float)(((double)y + 0.5) * g.sy - 0.5), g.h), tx = tap_at((float)(((double)xs + 0.5) * g.sx - 0.5), g.w);
    const uint8_t* r0 = g.img + (int64_t)ty.i0 * g.w * 3;
    const uint8_t* r1 = g.img + (int64_t)ty.i1 * g.w * 3;
    const int64_t c0 = (int64_t)tx.i0 * 3, c1 = (int64_t)tx.i1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (float)r0[c0 + c] * tx.w0 + (float)r0[c1 + c] * tx.w1;
        const float bot = (float)r1[c0 + c] * tx.w0 + (float)r1[c1 + c] * tx.w1;
        lvl[c] = rintf(top * ty.w0 + bot * ty.w1);   // nearest even; a convex blend of levels stays in 0 .. 255
    }
}

__global__ __launch_bounds__(256) void det_batch_kernel(
    const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off, const int32_t* __restrict__ src_hw,
    const int64_t* __restrict__ index, const int64_t* __restrict__ box_start, const int32_t* __restrict__ box_count, int64_t N,
    const float* __restrict__ boxes, const int64_t* __restrict__ labels, int64_t M, const double* __restrict__ draws, int flip_enabled,
    int B, int S1, int S, int new_h, int new_w, double s2y, double s2x, double ratio_y, double ratio_x, float* __restrict__ canvas,
    uint8_t* __restrict__ stage1, float* __restrict__ gt, int64_t gt_rows, int32_t* __restrict__ offsets) {
    __shared__ int part[256];
    const int b = blockIdx.y, t = threadIdx.x;
    const Geo g = geometry(src, src_bytes, src_off, src_hw, index, N, draws, flip_enabled, S1, b);

    // ---- the canvas pixel
    const int p = blockIdx.x * 256 + t;
    if (p < S * S) {
        const int y = p / S, x = p - y * S;
        float* o = canvas + ((size_t)b * S * S + p) * 3;
        if (!g.ok || y >= new_h || x >= new_w) {
            o[0] = o[1] = o[2] = 0.f;
        } else {
            const float mean[3] = {0.406f, 0.456f, 0.485f}, istd[3] = {0.225f, 0.224f, 0.229f};   // preprocess_kernel's
            const bool same = new_h == S1 && new_w == S1;
            Tap ty{y, y, 1.f, 0.f}, tx{x, x, 1.f, 0.f};
            if (!same) {
                ty = tap_at((float)fma((double)y + 0.5, s2y, -0.5), S1);
                tx = tap_at((float)fma((double)x + 0.5, s2x, -0.5), S1);
            }
            float l[4][3];
            stage1_pixel(g, ty.i0, tx.i0, l[0]);
            if (same) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (l[0][c] / 255.f - mean[c]) / istd[c];
            } else {
                const bool dx = tx.i1 != tx.i0, dy = ty.i1 != ty.i0;   // a clamped tap is the pixel already computed
                if (dx) stage1_pixel(g, ty.i0, tx.i1, l[1]);
                if (dy) stage1_pixel(g, ty.i1, tx.i0, l[2]);
                if (dx && dy) stage1_pixel(g, ty.i1, tx.i1, l[3]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (!dx) l[1][c] = l[0][c];
                    if (!dy) l[2][c] = l[0][c];
                    if (!dy) l[3][c] = l[1][c];
                    else if (!dx) l[3][c] = l[2][c];
                    float v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = (l[q][c] / 255.f - mean[c]) / istd[c];
                    const float top = fmaf(v[1], tx.w1, v[0] * tx.w0), bot = fmaf(v[2], tx.w0, v[3] * tx.w1);
                    o[c] = top * ty.w0 + bot * ty.w1;
                }
            }
        }
    }

    // ---- the stage-1 image, on request: this image's workgroups stride over its S1 x S1 pixels
    if (stage1 != nullptr) {
        const int n1 = S1 * S1;
        for (int q = blockIdx.x * 256 + t; q < n1; q += gridDim.x * 256) {
            const int y = q / S1, x = q - y * S1;
            float l[3] = {0.f, 0.f, 0.f};
            if (g.ok) stage1_pixel(g, y, x, l);
            uint8_t* o = stage1 + ((size_t)b * n1 + q) * 3;
            o[0] = (uint8_t)l[0], o[1] = (uint8_t)l[1], o[2] = (uint8_t)l[2];
        }
    }

    // ---- the ground-truth rows of this image, by its first workgroup
    if (blockIdx.x != 0) return;
    int before = 0, all = 0;   // rows of the images before b / of the whole batch
    for (int i = t; i < B; i += 256) {
        const int64_t row = index[i], off = src_off[i];
        const int h = src_hw[2 * i], w = src_hw[2 * i + 1];
        const bool ok = row >= 0 && row < N && h >= 1 && w >= 1 && off >= 0 && off <= src_bytes && (int64_t)h * w <= (src_bytes - off) / 3;
        const int n = ok ? max(box_count[row], 0) : 0;
        all += n;
        if (i < b) before += n;
    }
    for (int pass = 0; pass < 2; ++pass) {   // integer sums: any order gives the same result
        part[t] = pass ? all : before;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) part[t] += part[t + s];
            __syncthreads();
        }
        if (pass) all = part[0];
        else before = part[0];
        __syncthreads();
    }
    if (t == 0) offsets[b] = before;
    if (b == B - 1) {
        if (t == 0) offsets[B] = all;
        for (int64_t r = (int64_t)all + t; r < gt_rows; r += 256)
            for (int k = 0; k < 5; ++k) gt[r * 5 + k] = 0.f;
    }
    if (!g.ok) return;
    const int64_t row = index[b];
    const int64_t start = box_start[row];
    const int n = max(box_count[row], 0);
    const float edge = (float)(g.rw - 1);
    for (int i = t; i < n; i += 256) {
        const int64_t s = start + i, d = (int64_t)before + i;
        if (s < 0 || s >= M || d >= gt_rows) continue;
        float x1 = boxes[4 * s] * g.scale, y1 = boxes[4 * s + 1] * g.scale, x2 = boxes[4 * s + 2] * g.scale, y2 = boxes[4 * s + 3] * g.scale;
        if (g.flip) {
            const float fx1 = edge - x2, fx2 = edge - x1;
            x1 = fx1, x2 = fx2;
        }
        float* o = gt + d * 5;
        o[0] = (float)((double)x1 * ratio_x), o[1] = (float)((double)y1 * ratio_y);
        o[2] = (float)((double)x2 * ratio_x), o[3] = (float)((double)y2 * ratio_y);
        o[4] = (float)(double)(labels[s] - 1);
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_det_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int32_t* src_hw, const int64_t* index,
                             const int64_t* box_start, const int32_t* box_count, int64_t N, const float* boxes, const int64_t* labels,
                             int64_t M, const double* draws, int flip_enabled, int B, int S1, int S, float* canvas, uint8_t* stage1,
                             float* gt, int64_t gt_rows, int32_t* offsets, void* stream) {
    if (B == 0) return 0;
    STL_CHECK(B > 0 && B <= STL_DET_BATCH_MAX, "det_batch: %d images (at most %d)", B, STL_DET_BATCH_MAX);
    STL_CHECK(S1 >= 1 && S1 <= STL_DET_BATCH_SIDE && S >= 1 && S <= STL_DET_BATCH_SIDE, "det_batch: S1 %d, canvas %d (1 .. %d)", S1, S,
              STL_DET_BATCH_SIDE);
    STL_CHECK(N >= 0 && M >= 0 && src_bytes >= 0 && gt_rows >= 0, "det_batch: N %lld M %lld src_bytes %lld gt_rows %lld", (long long)N,
              (long long)M, (long long)src_bytes, (long long)gt_rows);
    STL_CHECK(src && src_off && src_hw && index && canvas && offsets, "det_batch: null pointer");
    STL_CHECK(N == 0 || (box_start && box_count), "det_batch: null annotation table");
    STL_CHECK(M == 0 || (boxes && labels), "det_batch: null box table");
    STL_CHECK(gt_rows == 0 || gt, "det_batch: null gt");
    // aspectaware_resize_padding's sizes of an S1 x S1 image on an S canvas (efficientdet.resize_meta: old_w > old_h is false)
    const int new_w = (int)((double)S / (double)S1 * (double)S1), new_h = S;
    STL_CHECK(new_w >= 1 && new_w <= S, "det_batch: S1 %d on canvas %d resizes to width %d", S1, S, new_w);
    const double ratio_x = (double)new_w / (double)S1, ratio_y = (double)new_h / (double)S1;
    STL_LAUNCH(det_batch_kernel, dim3(ceil_div(S * S, 256), B), dim3(256), 0, ST, src, src_bytes, src_off, src_hw, index, box_start,
               box_count, N, boxes, labels, M, draws, flip_enabled, B, S1, S, new_h, new_w, 1.0 / ratio_y, 1.0 / ratio_x, ratio_y,
               ratio_x, canvas, stage1, gt, gt_rows, offsets);
    STL_LAUNCH_CHECK("det_batch");
    return 0;
}
