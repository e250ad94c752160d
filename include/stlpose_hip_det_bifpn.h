/*
 * stlpose_hip_det_bifpn.h -- the backward of the EfficientDet BiFPN node (stlpose_amd/csrc/detector_bifpn.hip): the adjoint of
 * stl_det_fuse, i.e. of _forward_fast_attention (models/efficientdet_utils/model.py:181-253) as this library states it, and the
 * gradient add that joins the two heads' contributions to a level, and the adjoint of the first cell's plain pooled maps.  With the four backward entry points of the heads'
 * separable convs (stl_det_pointwise_bwd_weight / _data, stl_det_dwconv_bwd_weight / _data in stlpose_hip.h) these are all the
 * launches of a trainable BiFPN cell's backward (stlpose_amd/detector_train.py).  fp32 only.  Part of libstlpose_hip.so; written
 * in the C subset of stlpose_hip.h and read by the same reader (stlpose_amd/capi.py), which takes StlDetFuse from that header.
 */
#ifndef STLPOSE_HIP_DET_BIFPN_H
#define STLPOSE_HIP_DET_BIFPN_H
#include <stdint.h>
#include "stlpose_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Per term of the forward node: dx[i] NULL -- the term is frozen, nothing is computed for it and nothing is written; otherwise
 * fp32 of the term's own shape [B, t[i].H, t[i].W, C], written (accumulate[i] 0) or added to (accumulate[i] 1). */
typedef struct {
    float* dx[3];
    int32_t accumulate[3];
    int32_t pad_;
} StlDetFuseBwd;

/* Backward of stl_det_fuse with fast attention (f->wparam not NULL): out = swish(s), s = sum_i w^_i read_i, w^_i = relu(p_i) /
 * (sum_j relu(p_j) + 1e-4).  f is the forward's descriptor (f->out is not read: s is recomputed from the terms with the forward's
 * expression and order); dy fp32 [B, H, W, C] is the gradient of the node's output.
 *   ds     = dy * swish'(s)
 *   dwhat  fp32 [nterms]: dw^_i = sum_{b, y, x, c} ds * read_i -- fp64 partial sums per workgroup, added in partial order, rounded once
 *   dx[i]  in gather form, one thread per element of term i's own map (no atomics):
 *            mode 0  w^_i * ds
 *            mode 1  w^_i * (the sum of the up to four ds this pixel was read by, row-major; clipped at H, W: the term may be
 *                    ceil(H / 2) x ceil(W / 2), so an odd output is allowed here although stl_det_fuse takes even ones only)
 *            mode 2  over the up to four pool windows that hold the pixel, row-major: + w^_i * ds[window] if the pixel is the
 *                    window's winner by the forward's scan (first strict maximum in (ky, kx) order, padded taps 0 at their
 *                    places); a window won by a padded tap gives its gradient to nobody
 * The raw parameters' gradients follow from dwhat on the host side (relu and the normalisation; detector_train.fusion_weight_grads).
 * workspace: stl_det_fuse_bwd_workspace(B * H * W * C) floats, 8-byte aligned.  dy, the workspace and the dx may not overlap each
 * other or the terms.  One launch for ds, dwhat's partial sums and the mode-0 dx, one for dwhat, one per requested term of mode
 * 1 or 2.  Every sum runs in a fixed order: two runs give bitwise equal results. */
int stl_det_fuse_bwd(const StlDetFuse* f, const float* dy, const StlDetFuseBwd* g, float* workspace, float* dwhat, void* stream);
int64_t stl_det_fuse_bwd_workspace(int64_t n);

/* Backward of stl_det_fuse without weights (f->wparam NULL: a plain resample) of one mode-2 term: the pooled maps of the first
 * BiFPN cell, t -> p6 and p6 -> p7 (p5_to_p6's and p6_to_p7's MaxPool2dStaticSamePadding).  f is the forward's descriptor; dy fp32
 * [B, H, W, C] is the gradient of the pooled map, dx fp32 [B, t[0].H, t[0].W, C] that of its input, written (accumulate 0) or
 * added to (accumulate 1).  The contract of stl_det_fuse_bwd's mode-2 dx with w^ = 1 and ds = dy, by the same routine: gather form,
 * over the up to four windows that hold the pixel, row-major, + dy[window] if the pixel is the window's winner by the forward's scan
 * (first strict maximum in (ky, kx) order, padded taps 0 at their places); a window won by a padded tap gives its gradient to
 * nobody.  One thread per four channels where C % 4 == 0 and t[0].x, dy and dx are 16-byte aligned, per channel otherwise.  No
 * atomics: two runs give bitwise equal results.  dy and dx may not overlap.  One launch.  (A separate entry point:
 * stl_det_fuse_bwd takes weighted nodes only.) */
int stl_det_pool_bwd(const StlDetFuse* f, const float* dy, float* dx, int accumulate, void* stream);

/* out[e] = sa * a[e] + sb * b[e] for n elements, a first; sa / sb: one fp32 on the device each, NULL for 1.  out may be a or b.
 * The two heads' gradients of a level (regressor first), each times the gradient of its own loss. */
int stl_det_grad_add(const float* a, const float* b, const float* sa, const float* sb, float* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
