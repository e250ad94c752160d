// The per-batch tail of the evaluation on gfx950: what src/03_evaluate.py does with a batch's heat maps between the network and
// the epoch's scoring (flip_back + average, loss, the two arg-max of the PCK, quarter-pixel decode), as ONE pass over the maps
// that writes a few numbers per (person, joint) into tables the epoch keeps on the device, so that the host never waits for a batch.
//
//   stl_eval_tail     one workgroup per (person b, joint j).  Reads the two raw network outputs and the target once; forms the
//                     merged value of flip_merge_kernel in registers (never stored), its arg-max and that of the target
//                     (better() of common.cuh: NaN first, ties to the smaller index), the quarter-pixel refinement of
//                     final_preds_kernel from the four neighbours (recomputed from the two sources) and the fp64 sum of the
//                     squared weighted error of mse_kernel.
//   stl_eval_affine   once per epoch over all rows: the inverse crop transform of final_preds_kernel on the refined coordinates.
//
// Exactness.  fp contract is off for this file.  Every element step is the fp32 expression of the kernel it replaces, so arg-max,
// coordinates and maxval equal those of flip_merge -> heatmap_argmax / final_preds bit for bit.  The squared error is summed in
// fp64 in a fixed order (thread: ascending index with stride 256; wave: xor butterfly 32, 16, .. 1; block: wave 0 + 1 + 2 + 3),
// the same on every run; it is not the order of mse_kernel, whose grid-stride sum it replaces: all terms are non-negative, so
// the two fp64 sums agree to n * 2^-53 relative and the fp32 loss to one ulp.
#include "common.cuh"

#pragma clang fp contract(off)

namespace {

// merged[y][x] of flip_merge_kernel for one map: a = this joint's map, bf = the mirrored pass's map of joint perm[j] (or null)
__device__ __forceinline__ float merged_at(const float* a, const float* bf, int y, int x, int W) {
    const float v = a[y * W + x];
    if (!bf) return v;
    const int xs = x > 0 ? x - 1 : 0;   // 1-px right shift, column 0 keeps its own value
    return 0.5f * (v + bf[y * W + (W - 1 - xs)]);
}

__global__ __launch_bounds__(256) void eval_tail_kernel(const float* __restrict__ a, const float* __restrict__ bflip,
                                                        const int32_t* __restrict__ perm, const float* __restrict__ target,
                                                        const float* __restrict__ tweight, float* pred_xy, float* tgt_xy,
                                                        float* coords, float* maxval, double* partial, int J, int H, int W) {
    __shared__ float sv[4], tv[4];
    __shared__ int si[4], ti[4];
    __shared__ double sred[4];
    const int bj = blockIdx.x, j = bj % J, HW = H * W;
    const float* ra = a + (size_t)bj * HW;
    const float* rt = target + (size_t)bj * HW;
    const float* rb = nullptr;
    if (bflip) {
        int pj = perm[j];
        if ((unsigned)pj >= (unsigned)J) pj = j;   // a map outside the table is never read
        rb = bflip + ((size_t)(bj - j) + pj) * HW;
    }
    const float w = tweight[bj];
    float bv = -INFINITY, cv = -INFINITY;
    int bi = 0x7fffffff, ci = 0x7fffffff;
    double acc = 0.0;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const int y = i / W;
        const float m = merged_at(ra, rb, y, i - y * W, W);
        const float t = rt[i];
        argmax_take(m, i, bv, bi);
        argmax_take(t, i, cv, ci);
        const float d = (m - t) * w;
        acc += (double)d * (double)d;
    }
    block_argmax_reduce(bv, bi, sv, si);
    block_argmax_reduce(cv, ci, tv, ti);
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[bj] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
        const float m = bv > 0.f ? 1.f : 0.f;
        float cx = (float)(bi % W) * m, cy = (float)(bi / W) * m;
        pred_xy[2 * bj] = cx, pred_xy[2 * bj + 1] = cy;
        const float tm = cv > 0.f ? 1.f : 0.f;
        tgt_xy[2 * bj] = (float)(ci % W) * tm, tgt_xy[2 * bj + 1] = (float)(ci / W) * tm;
        const int px = (int)floorf(cx + 0.5f), py = (int)floorf(cy + 0.5f);
        if (1 < px && px < W - 1 && 1 < py && py < H - 1) {
            const float dx = merged_at(ra, rb, py, px + 1, W) - merged_at(ra, rb, py, px - 1, W);
            const float dy = merged_at(ra, rb, py + 1, px, W) - merged_at(ra, rb, py - 1, px, W);
            cx += (dx > 0.f) ? 0.25f : (dx < 0.f ? -0.25f : 0.f);
            cy += (dy > 0.f) ? 0.25f : (dy < 0.f ? -0.25f : 0.f);
        }
        coords[2 * bj] = cx, coords[2 * bj + 1] = cy;
        maxval[bj] = bv;
    }
}

__global__ __launch_bounds__(256) void eval_affine_kernel(const float* __restrict__ coords, const float* __restrict__ maxval,
                                                          const float* __restrict__ center, const float* __restrict__ scale,
                                                          float* preds, int64_t NJ, int J, int H, int W) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= NJ) return;
    const int64_t b = r / J;
    // inverse of the crop transform (rot = 0): scale s = W / (scale_x * 200) on both axes (final_preds_kernel's expression)
    const double s = (double)W / ((double)scale[2 * b] * 200.0);
    preds[3 * r] = (float)(((double)coords[2 * r] - 0.5 * W) / s + (double)center[2 * b]);
    preds[3 * r + 1] = (float)(((double)coords[2 * r + 1] - 0.5 * H) / s + (double)center[2 * b + 1]);
    preds[3 * r + 2] = maxval[r];
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_eval_tail(const float* a, const float* bflip, const int32_t* perm, const float* target, const float* tweight,
                             float* pred_xy, float* tgt_xy, float* coords, float* maxval, double* partial, int B, int J, int H, int W,
                             int64_t row0, void* stream) {
    if (B == 0 || J == 0) return 0;
    STL_CHECK(B > 0 && J > 0 && H > 0 && W > 0 && row0 >= 0, "eval_tail: B %d J %d H %d W %d row0 %lld", B, J, H, W, (long long)row0);
    STL_CHECK((int64_t)H * W <= (1 << 22), "eval_tail: map of %d x %d (at most 2^22 elements)", H, W);
    STL_CHECK((int64_t)B * J <= 0x7fffffff, "eval_tail: %d x %d maps in one batch", B, J);
    STL_CHECK(a && target && tweight && pred_xy && tgt_xy && coords && maxval && partial, "eval_tail: null pointer");
    STL_CHECK(!bflip || perm, "eval_tail: a mirrored output needs the joint permutation");
    const size_t o = (size_t)row0 * J;
    STL_LAUNCH(eval_tail_kernel, dim3(B * J), dim3(256), 0, ST, a, bflip, perm, target, tweight, pred_xy + 2 * o, tgt_xy + 2 * o,
               coords + 2 * o, maxval + o, partial, J, H, W);
    STL_LAUNCH_CHECK("eval_tail");
    return 0;
}

extern "C" int stl_eval_affine(const float* coords, const float* maxval, const float* center, const float* scale, float* preds,
                               int64_t N, int J, int H, int W, void* stream) {
    if (N == 0 || J == 0) return 0;
    STL_CHECK(N > 0 && J > 0 && H > 0 && W > 0, "eval_affine: N %lld J %d H %d W %d", (long long)N, J, H, W);
    STL_CHECK(coords && maxval && center && scale && preds, "eval_affine: null pointer");
    const int64_t nj = N * J, nblk = (nj + 255) / 256;
    STL_CHECK(nblk <= 0x7fffffff, "eval_affine: %lld rows", (long long)N);
    STL_LAUNCH(eval_affine_kernel, dim3((unsigned)nblk), dim3(256), 0, ST, coords, maxval, center, scale, preds, nj, J, H, W);
    STL_LAUNCH_CHECK("eval_affine");
    return 0;
}
