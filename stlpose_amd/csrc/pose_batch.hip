// The per-person augmentation arithmetic of a training batch on gfx950: what data/JointsDataset.py:164-200 does between reading a
// person's record and warping the image (half-body crop, scale / rotation / flip draws, the crop matrix, the joints through it),
// as ONE launch per batch over person tables that stay on the device.  The warp itself is stl_affine_crop and the heat maps are
// stl_gaussian_targets; this kernel writes exactly what those two read (minv, flip; float32 joints, visibility).
//
//   stl_pose_augment   one thread per person of the batch.  A person is 17 joints and a 3 x 3 fit: the kernel is bound by launch
//                      latency, not by arithmetic, so there is nothing to share between lanes and no LDS.
//
// The kernel draws nothing: the six random numbers per person come in as a table (pose_data.PoseBatchLoader makes them with a
// seeded device generator), so the kernel is a pure function of its inputs and a host replay checks it value by value.
//
// Exactness.  fp contract is off for this file.  Every step is the expression of the host function it replaces, in that
// function's number format (augment.half_body_transform: float32; the scale product, the centre flip, fliplr_joints, the control
// points before rounding, affine_points: float64), so flip, centre, scale, rotation, visibility and -- given the matrix -- the
// joints equal the host's bit for bit.  sin / cos of the rotation are the device library's: they may differ from the host's in the
// last digit, which moves a control point only when it lies on a float32 rounding boundary.  The three-point fit is a closed form
// (Cramer's rule) instead of the host's LU solve.  The control points are float32 values, so every product of two of them is exact
// in float64; the remaining sums, products and quotients are carried as unevaluated sums of two doubles (two_sum / two_prod /
// fma residuals), and each of the six entries is rounded to float64 once at the end.
#include "common.cuh"

#pragma clang fp contract(off)

namespace {

constexpr int J = 17;                                                     // COCO person keypoints
__device__ const int kFlipPerm[J] = {0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15};   // CONSTANTS.py:65 FLIP_PAIRS
constexpr int kUpperLast = 10;                                            // UPPER_BODY_IDS = 0 .. 10, the rest is the lower body

struct dd {   // hi + lo, |lo| <= ulp(hi) / 2
    double hi, lo;
};

__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return two_sum(s.hi, s.lo);
}
__device__ __forceinline__ dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
__device__ __forceinline__ dd dd_mul_d(dd a, double b) {   // (hi + lo) * b
    dd p = two_prod(a.hi, b);
    p.lo += a.lo * b;
    return two_sum(p.hi, p.lo);
}
__device__ __forceinline__ dd dd_div(dd n, dd d) {
    const double q1 = n.hi / d.hi;
    // n - q1 * d, the leading product exactly
    const double r = (fma(-q1, d.hi, n.hi) + n.lo) - q1 * d.lo;
    return two_sum(q1, r / d.hi);
}

// The exact-in-float64 affine map through three point pairs (x_i, y_i) -> (u_i, v_i), all float32 values: rows [a b c] of t with
// a * x_i + b * y_i + c = u_i.  Differences of float32 values are exact in float64 as long as their exponents lie within 29 of
// each other, which coordinates of one image always do; products of two such differences are then exact or carried by two_prod.
__device__ void fit3(const float* px, const float* py, const float* qu, const float* qv, double* t) {
    const double x0 = px[0], y0 = py[0];
    const double e1x = (double)px[1] - x0, e1y = (double)py[1] - y0, e2x = (double)px[2] - x0, e2y = (double)py[2] - y0;
    const dd det = dd_add(two_prod(e1x, e2y), dd_neg(two_prod(e1y, e2x)));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float* q = k ? qv : qu;
        const double u0 = q[0], d1 = (double)q[1] - u0, d2 = (double)q[2] - u0;
        const dd a = dd_div(dd_add(two_prod(d1, e2y), dd_neg(two_prod(d2, e1y))), det);
        const dd b = dd_div(dd_add(two_prod(e1x, d2), dd_neg(two_prod(e2x, d1))), det);
        const dd c = dd_add(dd{u0, 0.0}, dd_neg(dd_add(dd_mul_d(a, x0), dd_mul_d(b, y0))));
        t[3 * k] = a.hi, t[3 * k + 1] = b.hi, t[3 * k + 2] = c.hi;
    }
}

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }   // np.clip

__global__ __launch_bounds__(64) void pose_augment_kernel(
    const double* __restrict__ tjoints, const double* __restrict__ tvis, const float* __restrict__ tcenter,
    const float* __restrict__ tscale, const int32_t* __restrict__ twidth, int64_t N, const int64_t* __restrict__ index,
    const double* __restrict__ draws, int B, int train, int flip_enabled, double sf, double rf, int half_joints, double half_prob,
    int Wo, int Ho, double* center, double* scale, double* rot, int32_t* flip, double* trans, float* minv, double* joints,
    double* joints_vis, float* joints_xy, float* vis0) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t row = index[b];
    if (row < 0 || row >= N) {   // never read outside the tables: the row's results are NaN / 0 and the crop reads nothing
        const double nan = __builtin_nan("");
        center[2 * b] = center[2 * b + 1] = scale[2 * b] = scale[2 * b + 1] = rot[b] = nan;
        flip[b] = 0;
        for (int i = 0; i < 6; ++i) trans[6 * b + i] = nan, minv[6 * b + i] = 0.f;
        for (int i = 0; i < J * 3; ++i) joints[(size_t)b * J * 3 + i] = nan, joints_vis[(size_t)b * J * 3 + i] = 0.0;
        for (int i = 0; i < J; ++i) joints_xy[((size_t)b * J + i) * 2] = joints_xy[((size_t)b * J + i) * 2 + 1] = vis0[(size_t)b * J + i] = 0.f;
        return;
    }
    const double* jin = tjoints + (size_t)row * J * 3;
    const double* vin = tvis + (size_t)row * J * 3;
    const double* dr = draws + (size_t)b * 6;   // u_half, n_half, n_scale, u_rot, n_rot, u_flip
    float cf[2] = {tcenter[2 * row], tcenter[2 * row + 1]}, sfl[2] = {tscale[2 * row], tscale[2 * row + 1]};
    // the aspect ratio is a Python float on the host; against the float32 extents it is weak (numpy >= 2, NEP 50): the widening
    // below is float32 arithmetic with the ratio rounded to float32 first
    const float aspect = (float)((double)Wo * 1.0 / (double)Ho);

    // ---- half body (JointsDataset.py:166-171 + augment.half_body_transform)
    if (train) {
        double nvis = 0.0;
        int n_upper = 0, n_lower = 0;
        for (int j = 0; j < J; ++j) {
            nvis += vin[3 * j];
            if (vin[3 * j] > 0.0) (j <= kUpperLast ? n_upper : n_lower) += 1;
        }
        if (nvis > (double)half_joints && dr[0] < half_prob) {
            const bool upper = dr[1] < 0.5 && n_upper > 2;
            const int count = upper ? n_upper : n_lower;
            if (count >= 2) {
                float sx = 0.f, sy = 0.f, lox = INFINITY, loy = INFINITY, hix = -INFINITY, hiy = -INFINITY;
                for (int j = 0; j < J; ++j) {
                    if (!(vin[3 * j] > 0.0) || (j <= kUpperLast) != upper) continue;
                    const float x = (float)jin[3 * j], y = (float)jin[3 * j + 1];
                    sx += x, sy += y;                          // numpy's mean over axis 0: a running float32 sum in joint order
                    lox = fminf(lox, x), hix = fmaxf(hix, x), loy = fminf(loy, y), hiy = fmaxf(hiy, y);
                }
                float w = hix - lox, h = hiy - loy;
                if (w > aspect * h) h = w * 1.0f / aspect;
                else if (w < aspect * h) w = h * aspect;
                cf[0] = sx / (float)count, cf[1] = sy / (float)count;
                sfl[0] = (w * 1.0f / 200.0f) * 1.5f, sfl[1] = (h * 1.0f / 200.0f) * 1.5f;
            }
        }
    }

    // ---- scale, rotation, flip (JointsDataset.py:173-186)
    double c[2] = {(double)cf[0], (double)cf[1]}, s[2] = {(double)sfl[0], (double)sfl[1]}, r = 0.0;
    int fl = 0;
    if (train) {
        const double k = clipd(dr[2] * sf + 1.0, 1.0 - sf, 1.0 + sf);
        s[0] *= k, s[1] *= k;
        r = dr[3] <= 0.6 ? clipd(dr[4] * rf, -rf * 2.0, rf * 2.0) : 0.0;
        fl = flip_enabled && dr[5] <= 0.5;
    }
    const double width = (double)twidth[row];
    if (fl) c[0] = width - c[0] - 1.0;
    center[2 * b] = c[0], center[2 * b + 1] = c[1], scale[2 * b] = s[0], scale[2 * b + 1] = s[1], rot[b] = r, flip[b] = fl;

    // ---- crop matrix (augment.affine_matrices) and its inverse
    const double box_w = s[0] * 200.0, ang = 3.141592653589793 * r / 180.0, up = -0.5 * box_w;
    const double sn = sin(ang), cs = cos(ang);
    float px[3], py[3], qx[3], qy[3];
    px[0] = (float)c[0], py[0] = (float)c[1];
    px[1] = (float)(c[0] + (0.0 * cs - up * sn)), py[1] = (float)(c[1] + (0.0 * sn + up * cs));
    px[2] = px[1] + -(py[0] - py[1]), py[2] = py[1] + (px[0] - px[1]);       // the third point: float32 arithmetic
    const double wo = (double)Wo, ho = (double)Ho;
    qx[0] = (float)(wo * 0.5), qy[0] = (float)(ho * 0.5);
    qx[1] = (float)(wo * 0.5 + (double)0.0f), qy[1] = (float)(ho * 0.5 + (double)(float)(wo * -0.5));
    qx[2] = qx[1] + -(qy[0] - qy[1]), qy[2] = qy[1] + (qx[0] - qx[1]);
    double t[6];
    fit3(px, py, qx, qy, t);
    for (int i = 0; i < 6; ++i) trans[6 * b + i] = t[i];
    {   // inverse of [t; 0 0 1], rows 0 and 1, rounded to float32: crop pixel -> source coordinates
        const double det = t[0] * t[4] - t[1] * t[3];
        const double i00 = t[4] / det, i01 = -t[1] / det, i10 = -t[3] / det, i11 = t[0] / det;
        float* m = minv + 6 * b;
        m[0] = (float)i00, m[1] = (float)i01, m[2] = (float)(-(i00 * t[2] + i01 * t[5]));
        m[3] = (float)i10, m[4] = (float)i11, m[5] = (float)(-(i10 * t[2] + i11 * t[5]));
    }

    // ---- joints: fliplr_joints, then affine_points on what is visible (JointsDataset.py:185,198-200)
    double* jo = joints + (size_t)b * J * 3;
    double* vo = joints_vis + (size_t)b * J * 3;
    for (int j = 0; j < J; ++j) {
        const int sj = fl ? kFlipPerm[j] : j;
        const double v0 = vin[3 * sj], v1 = vin[3 * sj + 1], v2 = vin[3 * sj + 2];
        double x = jin[3 * sj], y = jin[3 * sj + 1], z = jin[3 * sj + 2];
        if (fl) x = (width - x - 1.0) * v0, y = y * v1, z = z * v2;
        if (v0 > 0.0) {
            const double nx = (x * t[0] + y * t[1]) + t[2], ny = (x * t[3] + y * t[4]) + t[5];
            x = nx, y = ny;
        }
        jo[3 * j] = x, jo[3 * j + 1] = y, jo[3 * j + 2] = z;
        vo[3 * j] = v0, vo[3 * j + 1] = v1, vo[3 * j + 2] = v2;
        joints_xy[((size_t)b * J + j) * 2] = (float)x, joints_xy[((size_t)b * J + j) * 2 + 1] = (float)y;
        vis0[(size_t)b * J + j] = (float)v0;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int stl_pose_augment(const double* joints_tab, const double* vis_tab, const float* center_tab, const float* scale_tab,
                                const int32_t* width_tab, int64_t N, const int64_t* index, const double* draws, int B, int train,
                                int flip_enabled, double scale_factor, double rot_factor, int num_joints_half_body,
                                double prob_half_body, int Wo, int Ho, double* center, double* scale, double* rot, int32_t* flip,
                                double* trans, float* minv, double* joints, double* joints_vis, float* joints_xy, float* vis0,
                                void* stream) {
    if (B == 0) return 0;
    STL_CHECK(B > 0 && N > 0 && Wo > 0 && Ho > 0, "pose_augment: B %d N %lld crop %d x %d", B, (long long)N, Wo, Ho);
    STL_CHECK(Wo <= (1 << 20) && Ho <= (1 << 20), "pose_augment: crop %d x %d (each side at most 2^20)", Wo, Ho);
    STL_CHECK(scale_factor >= 0.0 && rot_factor >= 0.0, "pose_augment: scale_factor %g rot_factor %g", scale_factor, rot_factor);
    STL_CHECK(joints_tab && vis_tab && center_tab && scale_tab && width_tab && index && draws, "pose_augment: null table");
    STL_CHECK(center && scale && rot && flip && trans && minv && joints && joints_vis && joints_xy && vis0, "pose_augment: null output");
    STL_LAUNCH(pose_augment_kernel, dim3((B + 63) / 64), dim3(64), 0, ST, joints_tab, vis_tab, center_tab, scale_tab, width_tab, N, index,
               draws, B, train, flip_enabled, scale_factor, rot_factor, num_joints_half_body, prob_half_body, Wo, Ho, center, scale, rot,
               flip, trans, minv, joints, joints_vis, joints_xy, vis0);
    STL_LAUNCH_CHECK("pose_augment");
    return 0;
}
