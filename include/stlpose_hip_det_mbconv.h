/*
 * stlpose_hip_det_mbconv.h -- the new pieces of an MBConv block's backward (stlpose_amd/csrc/detector_mbconv.hip): the
 * squeeze-excitation gate, the gated projection's input and the bias gradient of a depthwise layer that carries a folded BN
 * (MBConvBlock.forward, models/efficientnet/model.py:68-105, as this library runs it).  With the backward entry points of the
 * heads' separable convs (stl_det_pointwise_bwd_weight / _data, stl_det_dwconv_bwd_weight / _data in stlpose_hip.h) and
 * stl_det_grad_add (stlpose_hip_det_bifpn.h) these are all the launches of a trainable block's backward
 * (stlpose_amd/detector_train.py: ``model.set_train_backbone(k)`` trains the last k blocks of the backbone's final stage, k 3 / s 1
 * depthwise layers, with the BiFPN and the heads).  fp32 only, NHWC.  Part of libstlpose_hip.so; written in the C subset of
 * stlpose_hip.h and read by the same reader (stlpose_amd/capi.py).
 *
 * One block, with the folded weights the forward uses (e the expand layer's output, [B, HW, C] with C the expanded width):
 *   u = dwconv(e; w_d') + b_d'        a = swish(u)          p[b, c] = mean_hw a
 *   r = W1 p + b1   q = swish(r)      v = W2 q + b2         g = sigmoid(v)      (the forward's ``scale`` [B, C])
 *   y = (a * g) Wp' + bp' (+ the block input when the block has the skip)
 * Given D = dy Wp'^T [B, HW, C] (stl_det_pointwise_bwd_data):
 *   stl_det_mbconv_gate_bwd   xs = a * g (the x of the projection's weight gradient), asum[b, c] = sum_hw a, dgate[b, c] = sum_hw D a
 *   stl_det_se_bwd            dpool[b, c] = dL/dp, and the gradients of W1, b1, W2, b2
 *   stl_det_mbconv_act_bwd    du = (D g + dpool / HW) swish'(u), db_d'[c] = sum_{b, hw} du
 * Every sum runs in a fixed order (no float atomics): two runs give bitwise equal results.
 */
#ifndef STLPOSE_HIP_DET_MBCONV_H
#define STLPOSE_HIP_DET_MBCONV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The pixel ranges one image's HW pixels are split into by gate_bwd and act_bwd: one workgroup and one partial sum per (image,
 * range, 64 or 256 channels).  1 .. 16 up to 1024 pixels; above that ranges of 64 pixels, at most 1024 of them.
 * A change for direct callers: up to 1024 pixels the results and the workspace sizes are what they were, bit for bit; above 1024
 * pixels the count was 16 before, so the *_workspace queries return up to 64 times as much (call them again, do not keep an old
 * size) and asum, dgate and db come out in other bits, closer to the exact sums. */
int stl_det_mbconv_parts(int HW);

/* One pass over a and D [B, HW, C]: xs [B, HW, C] = a * g[b, c]; asum [B, C] = sum_hw a; dgate [B, C] = sum_hw D * a.  g [B, C].
 * A thread adds its pixels in order, the four waves of a workgroup are added in wave order, and a second launch adds the
 * stl_det_mbconv_parts(HW) partial sums of an image in range order (fp64, rounded once).  partial:
 * stl_det_mbconv_gate_bwd_workspace(B, HW, C) floats.  Four channels per thread where C % 4 == 0 and every pointer is 16-byte
 * aligned, one channel per thread otherwise.  xs may not overlap a or D.  Two launches. */
int stl_det_mbconv_gate_bwd(const float* a, const float* D, const float* g, float* xs, float* partial, float* asum, float* dgate, int B,
                            int HW, int C, void* stream);
int64_t stl_det_mbconv_gate_bwd_workspace(int B, int HW, int C);

/* Backward of stl_det_se from asum and dgate (stl_det_mbconv_gate_bwd) and the stored gate g [B, C]; w1 [Cs][C], b1 [Cs], w2 [C][Cs],
 * b2 [C] as the forward takes them (b2 is not read: g holds it).  Per image, with the forward's expressions: p = asum / HW, r = w1 p + b1, q = swish(r);
 * dv = dgate g (1 - g); dq = w2^T dv; dr = dq swish'(r); dpool [B, C] = w1^T dr (the gradient of p: act_bwd divides by HW).
 * Summed over the batch in image order: dw2 [C][Cs] = sum_b dv q^T, db2 [C] = sum_b dv, dw1 [Cs][C] = sum_b dr p^T, db1 [Cs] =
 * sum_b dr.  workspace: stl_det_se_bwd_workspace(B, C, Cs) floats.  (2 C + 2 Cs) floats of LDS: C + Cs <= 8192.  One workgroup per
 * image, then one launch for the four sums over the batch. */
int stl_det_se_bwd(const float* asum, const float* dgate, const float* g, int B, int HW, int C, int Cs, const float* w1, const float* b1,
                   const float* w2, const float* b2, float* workspace, float* dpool, float* dw1, float* db1, float* dw2, float* db2,
                   void* stream);
int64_t stl_det_se_bwd_workspace(int B, int C, int Cs);

/* du [B, HW, C] = (D * g[b, c] + dpool[b, c] / HW) * swish'(u), u the depthwise layer's pre-activation (stl_det_dwconv with act 0);
 * du may be D.  db [C] = sum_{b, hw} du: one partial sum per (image, pixel range) -- stl_det_mbconv_act_bwd_parts(B, HW) of them,
 * summed as in gate_bwd -- added in (image, range) order by a second launch (fp64, rounded once).  partial:
 * stl_det_mbconv_act_bwd_workspace(B, HW, C) floats.  The vector path as in gate_bwd.  Two launches; above 1024 pixels three: an
 * image's ranges first (fp64, kept as a float pair), then the images in order. */
int stl_det_mbconv_act_bwd(const float* D, const float* u, const float* g, const float* dpool, float* du, float* partial, float* db, int B,
                           int HW, int C, void* stream);
int64_t stl_det_mbconv_act_bwd_workspace(int B, int HW, int C);
int stl_det_mbconv_act_bwd_parts(int B, int HW);

/* ---- the rest of the trunk (stlpose_amd/csrc/detector_trunk.hip; ``model.set_train_trunk(k)`` trains the last k blocks of the whole
 * backbone, "all" the stem too): the depthwise backward for every kernel size and stride of the backbone, k in {3, 5}, s in {1, 2},
 * under the forward's TF "same" padding (stl_det_dwconv: before = max(0, (ceil(n / s) - 1) s - n + k) / 2 per axis), and the stem's
 * weight gradient.  Four channels per thread, 16 bytes per lane: C % 4 == 0 and 16-byte aligned tensors, anything else is an error
 * before a launch.  The 3 x 3 / 1 entry points of the heads (stl_det_dwconv_bwd_data / _weight, stlpose_hip.h) stay as they are. */

/* dx [B, H, W, C] = the adjoint of stl_det_dwconv(k, s) applied to dy [B, ceil(H / s), ceil(W / s), C], w [k][k][C]; times swish'(z), z
 * [B, H, W, C], where z is not NULL.  Gather form: one thread per (pixel of dx, 4 channels); s = 2 visits only the taps whose parity
 * matches the pixel's (at most 3 x 3 of the 25 at k = 5).  dx may not overlap dy or w.  One launch. */
int stl_det_dwconv_bwd_data_ks(const float* dy, const float* w, const float* z, float* dx, int B, int H, int W, int C, int k, int s,
                               void* stream);

/* dw [k][k][C] = sum over the OUTPUT pixels of x[the tap's input pixel] dy, x [B, H, W, C], dy [B, ceil(H / s), ceil(W / s), C].  One
 * partial sum per workgroup, stl_det_dwconv_bwd_ks_parts(B ceil(H / s) ceil(W / s)) pixel ranges (a thread adds every P-th pixel of its
 * range in order, the P pixel lanes of the workgroup are added in lane order), then a second launch adds the ranges in range order.
 * partial: parts k k C floats.  partial and dw may not overlap each other, x or dy.  Two launches. */
int stl_det_dwconv_bwd_weight_ks(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, int C, int k, int s,
                                 void* stream);
int stl_det_dwconv_bwd_ks_parts(int64_t npix);

/* The weight gradient of stl_det_stem (3 -> Co, 3 x 3 / 2, folded BN, swish): x the canvas [B, H, W, 3], w [3][3][3][Co] and bias [Co] as
 * the forward takes them, dy [B, ceil(H / 2), ceil(W / 2), Co] the gradient of the stem's output.  The pre-activation z of an output
 * pixel is recomputed from the canvas with the forward's expression; dz = dy swish'(z); dw [3][3][3][Co] = sum x dz, db [Co] = sum dz
 * through stl_det_stem_bwd_parts(B ceil(H / 2) ceil(W / 2)) ordered partial sums as above.  partial: parts 28 Co floats.  No image
 * gradient.  Two launches. */
int stl_det_stem_bwd(const float* x, const float* w, const float* bias, const float* dy, float* partial, float* dw, float* db, int B,
                     int H, int W, int Co, void* stream);
int stl_det_stem_bwd_parts(int64_t npix);

#ifdef __cplusplus
}
#endif
#endif
