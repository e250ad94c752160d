/*
 * stlpose_hip.h -- C ABI of libstlpose_hip.so (gfx950 / MI355X).
 *
 * The reference (angelvillar96/STLPose) has no FFI: its hot path is ATen/cuDNN ops invoked
 * from Python nn.Modules.  This header is the boundary the build creates for that path
 * (SURVEY.md 8(b) "What the native side must export").  Every entry point names the reference
 * computation it replaces.  Conventions:
 *   - plain pointers + sizes only; all tensor pointers are DEVICE pointers owned by the caller
 *     (the Python host allocates them with torch); kernels never allocate;
 *   - activations are NHWC ("channels last"), element type `dtype` = STL_F32 | STL_BF16 | STL_F16 (mixed 16-bit mode:
 *     forward tensors STL_F16, gradients STL_BF16, see STL_DT2 / ydtype), accumulation always fp32, BatchNorm statistics fp64;
 *   - every call enqueues on `stream` (a hipStream_t passed as void*) and returns without
 *     synchronising, so a whole step can be captured in a hipGraph;
 *   - return value 0 = ok, negative = error (message via stl_last_error()); the Python mirror
 *     raises RuntimeError like the reference's ATen calls would.
 */
#ifndef STLPOSE_HIP_H
#define STLPOSE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define STL_F32 0
#define STL_BF16 1
#define STL_F16 2 /* IEEE half: the FORWARD tensors (raw conv outputs, materialised sums, MFMA operands, kernel-layout weights of
                     the forward convs) of the mixed 16-bit mode -- BatchNorm bounds their range, and 10 mantissa bits instead of
                     bf16's 7 cut the distance from the fp32 reference 6-8 x at the same bytes and MFMA rate.
                     Gradients have no such bound and stay bf16: the backward kernels take the type of the forward tensors they
                     read (BatchNorm-backward source y, mask_y, mask_z, the weight gradient's h) as a second dtype, `ydtype`. */
#define STL_NSHARD 2 /* BatchNorm sum buffers are [STL_NSHARD][2*C] doubles (atomic de-contention).  Every consumer
                        reads all shards of its channels at the start of the launch (a dependent round trip in
                        front of ~800 launches per step): 8 / 4 / 2 / 1 shards = 16.25 / 15.89 / 15.65 / 15.87 ms */

/* How a tensor is read ("normalise on load"): a conv / sum kernel applies the producing
 * BatchNorm (+ReLU) while staging its input, so BN never costs its own pass over HBM. */
/* Two element types in one int argument: low byte = type of the gradient-side tensors, bits 8-15 = type of the forward-side
 * tensors when it differs (0 = the same).  stl_head_backward: (dx, x); stl_weight_prep*: (data-gradient layouts, forward layouts). */
#define STL_DT2(grad_dtype, fwd_dtype) ((grad_dtype) | ((fwd_dtype) << 8))

#define STL_SRC_PLAIN 0 /* v = x                                              */
#define STL_SRC_BN 1    /* v = [relu](a*x + b), a,b from batch or running stats  */
#define STL_SRC_BNBWD 2 /* v = a*(dt - r1/n - yhat*r2/n): BatchNorm backward on load */
#define STL_SRC_BNADD 3 /* v = [relu](a*x + b + y): a residual block end z = ReLU(BN(x) + y) (HRnet.py:58-59) formed while the
                           NEXT unit's first convolution stages its input; x = raw conv output, y = the skip tensor (same
                           shape, PLAIN).  stl_conv_forward only (3x3 stride 1, and 1x1 with Ci, Co >= 64: layer1's
                           bottleneck units, HRnet.py:88-100); with stl_conv.src_out the sum is also written out once, for the
                           skip connection and the backward pass */

typedef struct stl_src {
    const void* x;        /* PLAIN/BN: tensor; BNBWD: dt (grad wrt BN output, post ReLU mask) */
    const void* y;        /* BNBWD: raw conv output the BN normalised; BNADD: the tensor added after the BN */
    int32_t mode;         /* STL_SRC_*                                                    */
    int32_t relu;         /* BN: apply ReLU after the affine                              */
    const double* stats;  /* [NSHARD][2C] batch sum / sum-of-squares (train) or NULL (eval) */
    const double* rstats; /* BNBWD: [NSHARD][2C] r1 = sum dt, r2 = sum dt*yhat             */
    const float* gamma;   /* [C]                                                          */
    const float* beta;    /* [C]                                                          */
    const float* rmean;   /* [C] running mean (eval)                                      */
    const float* rvar;    /* [C] running var  (eval)                                      */
    float inv_count;      /* 1 / (B*H*W) of the normalised tensor                         */
    float eps;
} stl_src;

/* Implicit-GEMM convolution (no im2col), 3x3 pad 1 or 1x1 pad 0, MFMA 16x16 tiles.
 * Replaces nn.Conv2d forward (reference src/models/HRnet.py:26-29,69-75,146-150,201-205,
 * 219-223,290-294,352-356,371-373) and, with `transposed` weights, aten::convolution_backward's
 * data gradient.  out[b,oy,ox,co] = sum_{ky,kx,ci} src(b, oy*stride+ky-pad, ox*stride+kx-pad, ci)
 * * w[co][ky*ks+kx][ci].   stuff=1: the source is a stride-2 zero-stuffed view of a half-size
 * tensor (data gradient of a stride-2 conv).  Epilogue (all optional): +bias, +addend, ReLU
 * mask from the BatchNorm that produced this conv's input in the forward pass (mask_*),
 * ReLU, per-channel sum/sumsq of the stored output (out_stats) or r1/r2 against mask_y (red). */
typedef struct stl_conv {
    int32_t dtype;
    int32_t B, Hi, Wi, Ci; /* source tensor dims (for stuff=1: the half-size tensor) */
    int32_t Ho, Wo, Co;    /* output dims                                          */
    int32_t ks, stride, stuff;
    int32_t TH, TW;        /* output pixel tile; 0,0 = let stl_conv_plan choose      */
    int32_t shape;         /* block shape id chosen by stl_conv_plan (-1 = choose at launch) */
    stl_src src;
    const void* w;         /* [Co][ks*ks][Ci] dtype                               */
    void* out;             /* [B,Ho,Wo,Co] dtype                                  */
    const float* bias;     /* [Co] or NULL                                        */
    int32_t out_relu;
    double* out_stats;     /* [NSHARD][2*Co] += or NULL                           */
    const void* addend;    /* [B,Ho,Wo,Co] dtype or NULL                          */
    const void* mask_y;    /* [B,Ho,Wo,Co] raw tensor whose BN(+ReLU) gates `out`  */
    stl_src mask_bn;       /* BN parameters for mask_y (mode must be STL_SRC_BN)   */
    double* red;           /* [NSHARD][2*Co] += (r1,r2) against mask_y or NULL     */
    const void* mask_z;    /* [B,Ho,Wo,Co] dtype or NULL: ReLU output z whose sign gates `out` (out = 0 where
                              z <= 0).  With addend / mask_y (mask_bn.relu = 0) / red this is the backward of a
                              residual block end  z = ReLU(BN(y) + x)  fused into the data gradient that
                              produces the last contribution to dz (HRnet.py:58-59,99-100). */
    void* src_out;         /* BNADD source: [B,Hi,Wi,Ci] dtype -- the transformed source (the block-end sum) is stored here, every
                              pixel by the one block whose tile owns it; NULL = not stored */
    int32_t ydtype, math;       /* ydtype -- data gradient (BNBWD source) of the mixed mode: element type of the FORWARD tensors it reads
                              -- src.y, mask_y, mask_z -- when it differs from dtype (STL_F16 with dtype STL_BF16); 0 = same as dtype.
                              math -- STL_MATH_* (stlpose_hip_math.h): how the operands are multiplied; 0 (every zero-filled
                              descriptor) = natively, STL_MATH_BF16X3 = fp32 tensors on the bf16 matrix cores (forward launches) */
} stl_conv;
int stl_conv_forward(const stl_conv* p, void* stream);
/* Fill p->shape / p->TH / p->TW once (host-side tile search) so that launches are cheap. */
int stl_conv_plan(stl_conv* p);
/* 1 when stl_conv_forward has a kernel variant that takes p (already planned) with a STL_SRC_BNADD source. */
int stl_conv_bnadd_ok(const stl_conv* p);

/* Weight gradient of the same convolution (aten::convolution_backward, weight part).
 * partial[s][co][tap][ci] (fp32) for s < nsplit; summed later by stl_reduce_slabs.
 * h = the conv's forward input (PLAIN or BN source), g = gradient of its output (PLAIN or BNBWD). */
typedef struct stl_wgrad {
    int32_t dtype;
    int32_t B, Hi, Wi, Ci, Ho, Wo, Co, ks, stride;
    int32_t TH, TW, nsplit;
    stl_src h;
    stl_src g;
    float* partial; /* [nsplit][Co][ks*ks][Ci] */
    int32_t ydtype; /* mixed mode: element type of the forward tensors h.x and g.y (STL_F16) when dtype (g.x = dt, the MFMA operands)
                       is STL_BF16; 0 = same as dtype */
} stl_wgrad;
int stl_conv_wgrad(const stl_wgrad* p, void* stream);
/* Up to STL_WGRAD_GROUP_MAX weight gradients of IDENTICAL geometry, tile, nsplit and gradient-source mode in one
 * launch (grid.x = n * nsplit).  Same results as n stl_conv_wgrad calls; replaces n of the per-layer
 * aten::convolution_backward weight parts of one branch (HRnet.py:140-186: the 3x3 convolutions of
 * _make_one_branch share one shape). */
#define STL_WGRAD_GROUP_MAX 8
typedef struct stl_wgrad_io { stl_src h; stl_src g; float* partial; } stl_wgrad_io;
typedef struct stl_wgrad_group { int32_t n, pad_; const stl_wgrad* p[STL_WGRAD_GROUP_MAX]; } stl_wgrad_group;
int stl_conv_wgrad_group(const stl_wgrad_group* g, void* stream);
/* Channel tile (32 or 64) of the kernel variant stl_conv_wgrad uses for this problem: the grid is
 * nsplit x ceil(Co/tile) x ceil(Ci/tile) blocks, which is what a caller sizes nsplit against. */
int stl_wgrad_chunk(const stl_wgrad* p);

/* Sum of up to 4 terms + optional ReLU, each term read through an stl_src and optionally
 * nearest-upsampled by 2^shift.  Replaces the residual add+ReLU of the reference's blocks
 * (HRnet.py:58-59,99-100), the materialisation of transition outputs (:352-358,371-376) and the
 * multi-resolution exchange sum  out_i = ReLU(sum_j f_ij(x_j))  incl. nn.Upsample (:207,:255-264). */
typedef struct stl_term {
    stl_src src;
    int32_t shift; /* source is (H>>shift, W>>shift) */
} stl_term;
typedef struct stl_fuse {
    int32_t dtype, B, H, W, C, nterms, relu;
    stl_term t[4];
    void* out;
} stl_fuse;
int stl_fuse_forward(const stl_fuse* p, void* stream);

/* Backward of stl_fuse_forward: du = (sum_k dz_k) * (z > 0); for every same-resolution BN term
 * accumulates r1 = sum du, r2 = sum du*yhat into that term's rstats.  (aten::threshold_backward
 * + native_batch_norm_backward reductions.) */
typedef struct stl_fuse_bwd {
    int32_t dtype, B, H, W, C, ngrads, relu, nbn; /* dtype: the gradients dz / du */
    const void* dz[4];
    const void* z;
    void* du;
    stl_src bn[4];    /* same-res BN terms (mode STL_SRC_BN): x = raw y, stats, gamma */
    double* rstats[4];
    int32_t ydtype, pad_; /* mixed mode: element type of the forward tensors z and bn[].x (STL_F16 with dtype STL_BF16); 0 = dtype */
} stl_fuse_bwd;
int stl_fuse_backward(const stl_fuse_bwd* p, void* stream);

/* Backward of one nearest-upsampled BN term (upsample_nearest2d_backward + BN reductions):
 * dt[b,y,x,c] = sum over the 2^shift x 2^shift patch of du; r1/r2 against the low-res raw y. */
typedef struct stl_upbwd {
    int32_t dtype, B, H, W, C, shift; /* H,W = LOW-res dims */
    const void* du;                   /* [B, H<<shift, W<<shift, C] */
    void* dt;                         /* [B,H,W,C] */
    stl_src bn;
    double* rstats;
    int32_t ydtype, pad_; /* mixed mode: element type of bn.x (STL_F16 with dtype STL_BF16); 0 = dtype */
} stl_upbwd;
int stl_upsample_backward(const stl_upbwd* p, void* stream);

/* 3x3 patches of an NCHW fp32 image batch (3 channels) as a 32-wide NHWC tensor
 * (k = (ky*3+kx)*3 + c, zero for k >= 27 and outside the image), optionally ImageNet-normalised
 * first ((x-mean)/std, reference lib/loss.py:46-47).  Turns the 3-channel stem conv
 * (HRnet.py:290) / VGG conv1_1 into a 1x1 convolution with Ci=32. */
int stl_patch3x3(int dtype, const float* img, void* out, int B, int H, int W, int stride,
                 const float* mean3, const float* std3, void* stream);
/* Adjoint of stl_patch3x3 (the data gradient of the patch gather, elementwise.hip patch_kernel): dpatch = gradient of the
 * 32-wide patch tensor [B,Ho,Wo,32] (element type dtype; columns 27..31 are ignored) -> dimg fp32 NCHW [B,3,H,W], every
 * element written: dimg[b,c,iy,ix] = sum of dpatch[b,oy,ox,(ky*3+kx)*3+c] over the (oy,ox,ky,kx) with oy*stride+ky-1 = iy and
 * ox*stride+kx-1 = ix, divided by std3[c] if std3 != NULL (the normalised VGG stem; mean3 has no gradient).  Gather form in a
 * fixed order: no atomics, deterministic.  Gives the image gradient that autograd of the reference's stem conv
 * (HRnet.py:290, 434) returns for x. */
int stl_patch3x3_backward(int dtype, const void* dpatch, float* dimg, int B, int H, int W, int stride, const float* std3,
                          void* stream);

/* 1x1 head with bias: NHWC dtype [B,H,W,Ci] -> NCHW fp32 [B,J,H,W]  (HRnet.py:331-337,466).  J is 16 or 17 (the kernels keep a
 * pixel's J outputs in registers); forward: Ci % 8 == 0, Ci <= 512, bias may be NULL; backward: Ci % 16 == 0, Ci <= 64 (four
 * 16-column MFMA tiles) -- the widths of the network's head, 16 .. 64.  Anything else is refused before the launch. */
int stl_head_forward(int dtype, const void* x, const float* w, const float* bias, float* out,
                     int B, int H, int W, int Ci, int J, void* stream);
/* its backward: dx (dtype NHWC), per-block partials of dw [J][Ci] and db [J] (fp32): partial[nblk][J*Ci + J], every slab
 * written (zeros by a block that has no 256-pixel chunk).  dtype: STL_DT2(type of dx, type of x). */
int stl_head_backward(int dtype, const void* x, const float* w, const float* dout, void* dx,
                      float* partial, int nblk, int B, int H, int W, int Ci, int J, void* stream);

/* Gaussian heatmap targets on device (reference data/JointsDataset.py:230-286 generate_target):
 * joints_xy [B][J][2] in image pixels, vis [B][J] in {0,1} -> target [B][J][Hh][Wh] (unnormalised
 * gaussian, centre value 1, support 3*sigma, clipped at the border), tweight [B][J] (vis, or 0 when
 * the gaussian lies completely outside the map).  stride = image_size / heatmap_size per axis. */
int stl_gaussian_targets(const float* joints_xy, const float* vis, float* target, float* tweight, int B, int J,
                         int Hh, int Wh, float stride_x, float stride_y, float sigma, void* stream);

/* PersonMSELoss forward+backward (reference lib/loss.py:71-94):
 * loss = 0.5*mean(((o-t)*w)^2) over all B*J*H*W;  dout = (o-t)*w^2 / (B*J*H*W) * gscale.
 * loss == NULL: only dout and the per-block partial sums are written; the caller finishes the scalar with
 * stl_sum_partials(partial, nblk, 0.5 / (B*J*H*W), loss, 0, stream) whenever it likes (the train step: behind the
 * backward program, so that the one-block sum does not sit in front of the head's gradient). */
int stl_mse_loss(const float* out, const float* target, const float* tweight, float* dout,
                 double* partial, int nblk, float* loss, int B, int J, int HW, float gscale, void* stream);

/* get_max_preds_hrnet (reference lib/pose_parsing.py:16-55): first-max flat argmax + max per
 * (b,joint); idx int32 [B*J], maxval f32 [B*J], preds f32 [B*J*2] (x,y, zeroed when max<=0). */
int stl_heatmap_argmax(const float* hm, int32_t* idx, float* maxval, float* preds, int BJ, int H,
                       int W, void* stream);
/* flip_back + 1px shift + average of forward_pass(flip=True) (lib/inference.py:20-26,
 * lib/transforms.py:147-164) on device: out = 0.5*(a + shift(flip(b))). */
int stl_flip_merge(const float* a, const float* bflip, float* out, const int32_t* perm, int B, int J,
                   int H, int W, void* stream);
/* Adjoint of stl_flip_merge for gradient g of out (fp32 [B,J,H,W]): da = 0.5*g; dbf gathers 0.5*g through the joint
 * permutation, the mirror and the 1-px shift (column W-1 of dbf receives the terms of x = 0 and x = 1, column 0 none).
 * Gather form, deterministic; perm may be any map (every j with perm[j] = j' contributes to joint j'). */
int stl_flip_merge_backward(const float* g, float* da, float* dbf, const int32_t* perm, int B, int J, int H, int W,
                            void* stream);
/* +-0.25 px refinement + inverse affine of get_final_preds_hrnet (lib/pose_parsing.py:58-92). */
int stl_final_preds(const float* hm, const float* center, const float* scale, float* preds,
                    float* maxval, int B, int J, int H, int W, void* stream);

/* The per-batch tail of an evaluation in one pass over the maps (eval_tail.hip).  a, bflip, target fp32 [B, J, H, W]: the network's
 * output for the batch, its output for the mirrored batch (NULL: no flip test) and the target; perm int32 [J] as for
 * stl_flip_merge (an entry outside [0, J) reads the joint itself); tweight fp32 [B, J].  The merged map 0.5 * (a + shift(flip(bflip)))
 * of stl_flip_merge is formed in registers and not stored.  Written at rows row0 .. row0 + B - 1 of the caller's tables (the caller
 * keeps them large enough): pred_xy, tgt_xy fp32 [., J, 2]: the arg-max of the merged map and of the target as
 * stl_heatmap_argmax writes preds (zeroed where max <= 0); coords fp32 [., J, 2]: pred_xy after the +-0.25 px refinement of
 * stl_final_preds; maxval fp32 [., J].  partial fp64 [B * J] (not offset by row0): per map the sum of ((merged - target) * w)^2,
 * the difference in fp32, squares and sum in fp64 in a fixed order; the batch's PersonMSELoss is
 * stl_sum_partials(partial, B * J, 0.5 / (B * J * H * W), loss, 0, stream).  H * W <= 2^22. */
int stl_eval_tail(const float* a, const float* bflip, const int32_t* perm, const float* target, const float* tweight,
                  float* pred_xy, float* tgt_xy, float* coords, float* maxval, double* partial, int B, int J, int H, int W,
                  int64_t row0, void* stream);
/* Inverse crop transform of stl_final_preds over N table rows: preds fp32 [N, J, 3] = (x, y of coords [N, J, 2] in image
 * coordinates, maxval [N, J]); center, scale fp32 [N, 2]; H, W: the heat maps' size. */
int stl_eval_affine(const float* coords, const float* maxval, const float* center, const float* scale, float* preds, int64_t N,
                    int J, int H, int W, void* stream);

/* Table-driven batched helpers (one launch for the whole network). */
typedef struct stl_wprep { /* one conv weight: OIHW fp32 master -> kernel layouts */
    int64_t src_off;  /* element offset in master */
    int64_t fwd_off;  /* element offset in `wk`: [Co][tap][Cip] (Cip = padded Ci)          */
    int64_t bwd_off;  /* element offset in `wk`: [Ci][8-tap][Co] for the data gradient (patch: [tap*Ci + ci][Co], rows
                         Ci*ks*ks .. Cip-1 left as they are -- zero in a zero-initialised buffer), or -1 */
    int32_t Co, Ci, ks, Cip; /* Cip: Ci padded (stem patches: 27 -> 32)                     */
    int32_t patch;    /* 1: Ci*ks*ks flattened as k=(tap*Ci + ci) into Cip (stem / VGG conv1_1) */
    int32_t blk0;     /* first block of this entry */
} stl_wprep;
int stl_weight_prep(int dtype, const float* master, void* wk, const stl_wprep* tab, int n,
                    int nblocks, void* stream);

typedef struct stl_slab { /* one wgrad result: sum partial[s] -> grad (OIHW fp32) */
    int64_t part_off; /* element offset into `partials`; a multiple of 4 (16-byte aligned) when Ci % 4 == 0 */
    int64_t grad_off; /* element offset into `grads`    */
    int32_t nsplit, Co, Ci, ks, Cip, patch, blk0;
    int32_t pad; /* if non-zero: element stride between consecutive splits (default Co*taps*Ci) */
} stl_slab;
int stl_reduce_slabs(const float* partials, float* grads, const stl_slab* tab, int n, int nblocks,
                     void* stream);

typedef struct stl_bnrec { /* one BatchNorm layer */
    int64_t stats_off;  /* offset (doubles) of its [NSHARD][2C] block in the stats arena  */
    int64_t param_off;  /* offset of gamma in the fp32 master (beta follows at +C)        */
    int64_t buf_off;    /* offset of running_mean in the buffer arena (running_var at +C) */
    int32_t C;
    float inv_count;
} stl_bnrec;
/* running_mean/var momentum update (unbiased var), reference nn.BatchNorm2d(momentum=0.1).
 * overflow (device int32, NULL = off; the caller initialises it to INT32_MAX): range guard of the 16-bit forward tensors.  A raw
 * conv output beyond the storage type's range (STL_F16: |y| > 65504, e.g. a badly scaled checkpoint, lib/model_setup.py:38-42
 * loads arbitrary ones) is stored as infinity and shows in the layer's sums; such a layer keeps its running statistics --
 * EVERY channel of it, not only the channels whose sums are non-finite (with overflow == NULL too); num_batches_tracked still
 * counts the pass -- and the smallest index i of tab[] with non-finite sums is left in *overflow (atomic min).  A momentum of
 * 0 leaves the buffers bit-unchanged.  The count is rebuilt as 1 / (double)inv_count.  The optimisers below skip elements whose
 * gradient is not finite, so the step that overflowed leaves the weights as they were; the host reads the word when it reads
 * the loss (TrainStep.check_forward_range) and raises with the layer's name. */
int stl_bn_running_update(const double* stats, float* buffers, int64_t* num_batches_tracked /* [n] or NULL */,
                          const stl_bnrec* tab, int n, float momentum, int32_t* overflow, void* stream);
/* dgamma = r2, dbeta = r1 from the backward reduction arena into the flat grad buffer. */
int stl_bn_param_grads(const double* rstats, float* grads, const stl_bnrec* tab, int n, void* stream);

/* Optimisers over the flat fp32 master (torch.optim.Adam / SGD semantics, reference
 * lib/model_setup.py:135-141).  hyper = device float[8]: lr, beta1, beta2, eps, weight_decay,
 * momentum, nesterov, gscale;  step = device int32 (incremented by the kernel).  overflow: the word stl_bn_running_update
 * maintains -- when it reports a non-finite forward tensor the WHOLE step is skipped (step is left negative, not counted:
 * ReLU(NaN) = 0 can let the loss and the gradients of such a step come out finite and wrong); independently of it an element
 * whose gradient is NaN or infinite is left untouched (weight and moments). */
int stl_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                  int32_t* step, const int32_t* overflow /* or NULL */, void* stream);
int stl_sgd_step(float* p, const float* g, float* mom, int64_t n, const float* hyper, int32_t* step,
                 const int32_t* overflow /* or NULL */, void* stream);

/* Device affine crop + normalisation of a batch (reference data/JointsDataset.py:189-200: cv2.warpAffine(img,
 * get_affine_transform(c, s, r, image_size), INTER_LINEAR) followed by ToTensor + Normalize, data_loaders.py:59-61).
 * src: uint8 HWC RGB images packed in one buffer (src_off[b] bytes, src_hw[b] = (H, W)); minv[b] = the 2x3 matrix
 * that maps OUTPUT pixel (x, y) to source coordinates (the inverse of the reference's `trans`); flip[b] != 0 reads the
 * source mirrored left-right (the flip augmentation, :183-186); out = fp32 NCHW [B,3,Ho,Wo]; mean3/std3 may be NULL.
 * Bilinear taps outside the source contribute 0 (BORDER_CONSTANT).  cv2's 1/32-pixel fixed-point coordinate rounding
 * is NOT reproduced (exact float bilinear): parity for that rounding is unpinned (cv2 absent). */
int stl_affine_crop(const uint8_t* src, const int64_t* src_off, const int32_t* src_hw, const float* minv, const int32_t* flip,
                    float* out, int B, int Ho, int Wo, const float* mean3, const float* std3, void* stream);
/* The augmentation arithmetic of a training batch for COCO persons (17 joints; reference data/JointsDataset.py:164-200), one launch,
 * one thread per person, no allocation and no host read (pose_batch.hip).  Person tables of N rows: joints_tab, vis_tab fp64
 * [N, 17, 3]; center_tab, scale_tab fp32 [N, 2] (scale in units of 200 px); width_tab int32 [N]: the width of the person's source
 * image.  index int64 [B]: the table row of each person of the batch (a row may repeat); draws fp64 [B, 6] = u_half, n_half,
 * n_scale, u_rot, n_rot, u_flip (u: uniform in [0, 1), n: standard normal), made by the caller.  With train == 0 no draw is read:
 * rot 0, no flip, centre and scale as stored.  With train != 0, in this order:
 *   half body   iff sum(vis[:, 0]) > num_joints_half_body and u_half < prob_half_body: the visible joints 0 .. 10 iff n_half < 0.5
 *               and more than two of them are visible, else the visible joints 11 .. 16; with two or more selected, centre = their
 *               fp32 mean (running sum in joint order / count) and scale = their extent widened to Wo / Ho, / 200 * 1.5, all fp32;
 *   scale       (double)scale * clip(n_scale * scale_factor + 1, 1 - scale_factor, 1 + scale_factor);
 *   rot         clip(n_rot * rot_factor, -2 rot_factor, 2 rot_factor) iff u_rot <= 0.6, else 0 (degrees);
 *   flip        iff flip_enabled and u_flip <= 0.5: centre x = width - x - 1 (fp64), joints mirrored the same way, left / right
 *               pairs exchanged, joints multiplied by their visibility.
 * Outputs: center, scale fp64 [B, 2]; rot fp64 [B]; flip int32 [B]; trans fp64 [B, 2, 3]: the map image -> (Wo, Ho) crop through
 * the reference's three control points (rounded to fp32 as there; the fit itself is exact to the last digit of every entry); minv
 * fp32 [B, 6]: its inverse, what stl_affine_crop takes together with flip; joints, joints_vis fp64 [B, 17, 3]: the visible joints
 * through trans as (x * t00 + y * t01) + t02; joints_xy fp32 [B, 17, 2] and vis0 fp32 [B, 17]: what stl_gaussian_targets takes.
 * An index outside [0, N) reads nothing: that person's fp64 results are NaN, its flip, minv, visibility and fp32 joints 0. */
int stl_pose_augment(const double* joints_tab, const double* vis_tab, const float* center_tab, const float* scale_tab,
                     const int32_t* width_tab, int64_t N, const int64_t* index, const double* draws, int B, int train,
                     int flip_enabled, double scale_factor, double rot_factor, int num_joints_half_body, double prob_half_body,
                     int Wo, int Ho, double* center, double* scale, double* rot, int32_t* flip, double* trans, float* minv,
                     double* joints, double* joints_vis, float* joints_xy, float* vis0, void* stream);
/* VGG perceptual path (reference lib/loss.py:17-58). */
int stl_maxpool2x2(int dtype, const void* x, void* out, int B, int H, int W, int C, void* stream);
int stl_l1_partial(int dtype, const void* a, const void* b, int64_t n, double* partial, int nblk,
                   void* stream); /* partial[i] = sum |a-b| over block i's share */
/* Same with squared differences (content / Gram MSE of the VGG19 style loss, V2 -- no reference counterpart). */
int stl_l2_partial(int dtype, const void* a, const void* b, int64_t n, double* partial, int nblk, void* stream);
/* Image gradient of the VGG19 style loss (V2; stlpose_amd/vgg19_style.py, stylise.py).  Adjoint of stl_maxpool2x2
 * (max_pool2d backward, 2x2 / stride 2, floor mode): x = the pool's input [B,H,W,C], dy = gradient of its output
 * [B,H/2,W/2,C] -> dx [B,H,W,C], every element written.  Each window's gradient goes to its FIRST maximum in row-major order
 * (a later element wins only if strictly greater, or NaN: torch CPU's rule); the row / column an odd H / W drops gets 0;
 * mask != 0 also zeroes dx where x <= 0 (the ReLU in front of the pool, whose output x is).  Gather form: no atomics,
 * deterministic.  dtype STL_F32 or STL_BF16; C % 8 == 0. */
int stl_maxpool2x2_backward(int dtype, const void* x, const void* dy, void* dx, int B, int H, int W, int C, int mask, void* stream);
/* Adjoint of the content term at one tap, in place: g += scale[0] * (a - b) over n elements (n % 8 == 0), then, if mask != 0,
 * g = 0 where a <= 0 (the ReLU whose output a is).  scale is a DEVICE float (content weight of the backward pass * 2 / n of the
 * MSE), read by the kernel.  dtype STL_F32 or STL_BF16. */
int stl_l2_backward(int dtype, const void* a, const void* b, void* g, int64_t n, const float* scale, int mask, void* stream);
int stl_bilinear_nchw(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo,
                      void* stream); /* F.interpolate(mode='bilinear', align_corners=False) */
int stl_sum_partials(const double* partial, int n, double scale, float* out, int accumulate, void* stream);

/* Layout / dtype utilities. */
int stl_nchw_to_nhwc(int dtype, const float* in, void* out, int B, int C, int H, int W, void* stream);
int stl_nhwc_to_nchw(int dtype, const void* in, float* out, int B, int C, int H, int W, void* stream);

/* ---- native program replay (csrc/program.hip) --------------------------------------------------
 * The Python planner turns the network into a flat list of the calls above; stl_program_run()
 * enqueues all of them in one C call, on up to 16 HIP streams, with cross-stream RAW dependencies
 * expressed as events (wait[] = indices of earlier ops that record). */
#define STL_OP_CONV 0
#define STL_OP_WGRAD 1
#define STL_OP_FUSE 2
#define STL_OP_FUSE_BWD 3
#define STL_OP_UP_BWD 4
#define STL_OP_PATCH 5
#define STL_OP_HEAD 6
#define STL_OP_HEAD_BWD 7
#define STL_OP_REDUCE_RANGE 8 /* stl_reduce_slabs over a sub-range of the table (a gradient bucket) */
#define STL_OP_BN_GRADS_RANGE 9 /* stl_bn_param_grads over a sub-range of the table */
#define STL_OP_WGRAD_GROUP 10   /* stl_conv_wgrad_group */
/* 11 and 12 are retired (the in-program optimiser and weight re-layout): not reused */
#define STL_OP_PATCH_BWD 13    /* stl_patch3x3_backward (stl_patch_bwd): the image gradient of a plan with input gradients */
/* A gradient bucket = a contiguous slice of the flat gradient buffer whose weight-gradient slabs and
 * BatchNorm reductions are complete at some point of the backward program.  Reducing it there (and
 * recording an event) lets the data-parallel all-reduce of that slice start while the rest of
 * backward still runs (reference: the per-step gradient gather of nn.DataParallel, 02_train.py:109). */
typedef struct stl_reduce_range { const float* partials; float* grads; const stl_slab* tab; int32_t n, blk_base, nblocks, pad_; } stl_reduce_range;
typedef struct stl_bn_range { const double* rstats; float* grads; const stl_bnrec* tab; int32_t n, pad_; } stl_bn_range;
int stl_reduce_slabs_range(const stl_reduce_range* r, void* stream);
typedef struct stl_patch { int32_t dtype, B, H, W, stride, pad_; const float* img; void* out; const float* mean3; const float* std3; } stl_patch;
typedef struct stl_patch_bwd { int32_t dtype, B, H, W, stride, pad_; const void* dpatch; float* dimg; const float* std3; } stl_patch_bwd;
typedef struct stl_head { int32_t dtype, B, H, W, Ci, J; const void* x; const float* w; const float* bias; float* out; } stl_head;
typedef struct stl_head_bwd { int32_t dtype /* STL_DT2(dx, x) */, B, H, W, Ci, J, nblk, pad_; const void* x; const float* w; const float* dout; void* dx; float* partial; } stl_head_bwd;
typedef struct stl_op {
    int32_t kind;    /* STL_OP_*                                        */
    int32_t stream;  /* index into the streams array given to run()      */
    const void* desc; /* the op's descriptor struct (kept alive by the caller) */
    int32_t nwait;
    int32_t wait[8];
    int32_t record;  /* 1: record an event after this op (someone waits on it) */
} stl_op;
int stl_program_create(const stl_op* ops, int n, int nstreams, void** out_handle);
int stl_program_run(void* program, void* const* streams /* hipStream_t[nstreams]; [0] = main */);
/* Ops [first, last) only; first == 0 forks the side streams, last == n joins them.  A data-parallel host runs the backward program
 * bucket by bucket and enqueues each bucket's all-reduce between two ranges, i.e. right behind the bucket in every in-order queue. */
int stl_program_run_range(void* program, void* const* streams, int first, int last);
int stl_program_destroy(void* program);
/* Make `stream` wait for op `op` (which must record) of the LAST run of the program: how a
 * communication stream picks up a finished gradient bucket. */
int stl_program_wait_op(void* program, int op, void* stream);

/* Self-checks that need no reference: MFMA / LDS-transpose lane maps (used by tests). */
int stl_selftest_mfma(float* out /* [4] max abs err: bf16 mfma, f32 mfma, tr-read, f64 atomic */, void* stream);

/* ---- pose retrieval (stlpose_amd/csrc/retrieval.hip): the second half of the reference, src/06_fit_knn_tree.py and
 * src/07_retrieval_experiments.py.  Pose vectors are fp32 [N, D], D = 34 / 26 / 18 (STL_POSE_ALL_KPTS / FULL_BODY / UPPER_BODY).
 * Every kernel evaluates a (query, row) pair through one device routine with a fixed accumulation order (a sequential chain over
 * d = 0 .. D-1), so distances, top-k and rank agree bit for bit.  Result order: ascending distance, ties by ascending database
 * index, NaN last (np.argsort(kind="stable")). */
#define STL_POSE_ALL_KPTS 0   /* keypoints 0..16, D = 34 */
#define STL_POSE_FULL_BODY 1  /* keypoints 5..16, 0, D = 26 (the origin is the left shoulder, not the nose: the reference's order) */
#define STL_POSE_UPPER_BODY 2 /* keypoints 5..12, 0, D = 18 */
#define STL_POSE_EUCLIDEAN 0       /* pose_database.py:201-202 "euclidean_distance" */
#define STL_POSE_COSINE 1          /* :199-200 "cosine_similarity": 1 - x.y, no normalisation */
#define STL_POSE_MANHATTAN 2       /* :203-204 "manhattan_distance" */
#define STL_POSE_CONFIDENCE 3      /* :205-206, metrics.py:97-117 "confidence_score" (conf [Q, D], NULL = ones) */
#define STL_POSE_OKS 4             /* :207-210, metrics.py:120-149 "oks_score" (sigmas chosen by D) */
#define STL_POSE_L2SQ 5            /* hnswlib space "l2": squared L2 (penalization ignored) */
#define STL_POSE_COS_NORMALISED 6  /* hnswlib space "cosine": 1 - x.y / (|x| |y|) (penalization ignored) */
#define STL_POSE_PEN_ZERO_COORD 0  /* pose_database.py:226-229 */
#define STL_POSE_PEN_NONE 1        /* :231-236 |q| < 1e-5: q, row and confidence zeroed */
#define STL_POSE_PEN_MEAN 2        /* :238-243 |q| < 1e-5 and |row| > 1e-5: q = mean of the unmasked metric over rows 0..min(100,N)-1 */
#define STL_POSE_PEN_MAX 3         /*          ... = max of it (:251-285); computed per query inside the launch */
#define STL_POSE_TOPK_MAX 1024     /* largest k of stl_pose_topk */
#define STL_POSE_RANK_MAX 16384    /* largest N of stl_pose_rank: one workgroup holds N (dist, idx) keys in LDS (128 KiB) */
#define STL_POSE_RANK_LABELS_MAX 4 /* label levels scored by stl_pose_rank */
#define STL_POSE_RANK_ANY_MAX (1 << 24) /* largest N of stl_pose_rank_any: sorted runs of STL_POSE_RANK_MAX keys merged in global memory */
#define STL_POSE_NSCORES 10        /* p@1, p@5, p@10, p@rel, mAP, r@1, r@5, r@10, r@rel, mAR (metrics.py:25-94) */

/* joints [N, 17, C >= 2] (pose n at joints + n * row_stride, keypoint k at + k * C) -> out [N, D]: the selected keypoints' (x, y),
 * minus the first selected keypoint, entries that were exactly 0 kept 0, then (normalize) divided by max(L2 norm, 1e-5).
 * Replaces process_pose_vector (pose_database.py:19-69) and process_data (06_fit_knn_tree.py:84-147). */
int stl_pose_vectors(const float* joints, int64_t row_stride, int C, float* out, int N, int approach, int normalize, void* stream);
/* out [Q, N] = metric(q[i], db[j]) with the penalization of the query: the loop of get_neighbors_idxs (pose_database.py:220-245)
 * before its argsort.  Q <= 65535. */
int stl_pose_distances(const float* q, const float* conf, const float* db, float* out, int Q, int N, int D, int method,
                       int penalization, void* stream);
/* Bytes of the `work` buffer stl_pose_topk needs for (Q, N, k) (0: none), or a negative error code (k > N, k > STL_POSE_TOPK_MAX). */
int stl_pose_topk_workspace(int Q, int N, int k, int D);
/* Fused distance + top-k: idx int64 [Q, k], dist [Q, k], the first k of the ranking; never materialises [Q, N].  Replaces
 * get_neighbors_idxs with num_retrievals = k (pose_database.py:247-248) and hnswlib knn_query (:182-185, 06_fit_knn_tree.py:150-166)
 * exactly.  N is split across workgroups; a second launch merges the per-chunk lists. */
int stl_pose_topk(const float* q, const float* conf, const float* db, int Q, int N, int D, int method, int penalization, int k,
                  int64_t* idx, float* dist, void* work, int64_t work_bytes, void* stream);
/* Full ranking of N <= STL_POSE_RANK_MAX rows per query: the first k_out (0 .. N) indices / distances, and, when labels [L, N] is
 * given (with the queries' labels qlabels [L, Q], L <= 4), score_retrievals (metrics.py:25-94) of the first k_eff retrievals per
 * query and level into scores fp64 [Q, L, STL_POSE_NSCORES] (rank 0 dropped; all -1 when nothing relevant is retrieved;
 * 11 <= k_eff <= N).  The all-vs-all experiment (07_retrieval_experiments.py:67-112) without any [N, N] array. */
int stl_pose_rank(const float* q, const float* conf, const float* db, int Q, int N, int D, int method, int penalization, int k_out,
                  int64_t* idx, float* dist, const int32_t* labels, const int32_t* qlabels, int L, int k_eff, double* scores,
                  void* stream);
/* Bytes of the `work` buffer stl_pose_rank_any needs for (Q, N): two [Q, N] arrays of 8-byte keys above N = STL_POSE_RANK_MAX, a
 * token 16 bytes up to it.  Negative (error code) for Q < 0, N < 1 or N > STL_POSE_RANK_ANY_MAX. */
int64_t stl_pose_rank_any_workspace(int Q, int N);
/* stl_pose_rank for every 1 <= N <= STL_POSE_RANK_ANY_MAX: same arguments, checks, order and scores.  Up to STL_POSE_RANK_MAX rows
 * it runs stl_pose_rank itself; above, each query's keys are sorted in runs of STL_POSE_RANK_MAX in LDS, the runs merged pairwise
 * in `work` (merge path, ceil(log2(runs)) passes), and the scores computed from the sorted keys with stl_pose_rank's arithmetic in
 * a fixed summation order.  Q <= 65535 per call above STL_POSE_RANK_MAX; `work` 8-byte aligned; a missing or short workspace is
 * refused before anything is launched. */
int stl_pose_rank_any(const float* q, const float* conf, const float* db, int Q, int N, int D, int method, int penalization, int k_out,
                      int64_t* idx, float* dist, const int32_t* labels, const int32_t* qlabels, int L, int k_eff, double* scores,
                      void* work, int64_t work_bytes, void* stream);

/* ---- top-down pose extraction (stlpose_amd/csrc/topdown.hip): person boxes -> crops -> HRNet -> poses, the glue of
 * src/04_evaluate_vases_qualitatively.py:184-250 and src/05_create_archdata_retrieval_db.py:114-171. */
#define STL_BOX_MAX 4096           /* boxes per image of stl_box_select: one workgroup sorts them in LDS (~100 KiB) */
#define STL_RESIZE_SRC_MAX 16384   /* H * W of a source map of stl_heatmap_resize_argmax: staged in LDS (64 KiB) */
#define STL_RESIZE_DST_MAX 2048    /* each output side of stl_heatmap_resize_argmax (per-row / per-column taps in LDS) */

/* Per-image filter + greedy NMS for a ragged batch, one workgroup per image.  boxes fp32 [N, 4] (x1, y1, x2, y2), scores [N],
 * labels int64 [N] (NULL: no label test), offsets int64 [I + 1]: image i owns rows offsets[i] .. offsets[i+1]-1 (at most max_n <=
 * STL_BOX_MAX of them; an image above max_n gets count -1 and no output).
 * Filter (bbox_filtering, lib/bounding_box.py:127-168): a row passes when labels == label and (score_test) score > score_thr.
 * iou_thr < 0: filter only, the passing rows in input order.  Otherwise torchvision.ops.nms (as bbox_nms, :171-206, calls it) on
 * the passing rows: stable descending score order (NaN first), area = (x2-x1)*(y2-y1), iou = inter / (area_i + area_j - inter)
 * in fp32 left to right, a row suppressed when (double)iou > iou_thr; the survivors in score order.
 * keep int32 [N]: per image segment the image-local row indices of the kept rows, then -1; count int32 [I]. */
int stl_box_select(const float* boxes, const float* scores, const int64_t* labels, const int64_t* offsets, int num_images,
                   int64_t N, int max_n, int64_t label, int score_test, float score_thr, double iou_thr, int32_t* keep,
                   int32_t* count, void* stream);
/* F.interpolate(hm, (Ho, Wo), mode="bilinear", align_corners=True) followed by get_max_preds_hrnet (lib/pose_parsing.py:16-55),
 * fused: the upsampled maps are never written.  hm fp32 [BJ, H, W]; idx int32 [BJ] (flat index into Ho x Wo, may be NULL),
 * maxval [BJ], preds [BJ, 2] = (idx % Wo, idx / Wo) * (maxval > 0).  Torch's sample rule (scale = float(H-1)/(Ho-1), W first
 * within a row, then the rows) and stl_heatmap_argmax's order (NaN first, then larger, ties to the smaller index). */
int stl_heatmap_resize_argmax(const float* hm, int BJ, int H, int W, int Ho, int Wo, int32_t* idx, float* maxval, float* preds,
                              void* stream);

/* ---- COCO box AP (stlpose_amd/csrc/box_ap.hip, coco_match.inc): the validation metric of src/02_train_faster_rcnn.py:241-280 and
 * src/03_evaluate_faster_rcnn.py:119-184, i.e. the published COCOeval(..., "bbox") in two steps.  Exact: fp64 as written in that
 * file's head, integer sums, order-free maxima; tests/box_ap_ref.py reproduces both outputs bit for bit. */
#define STL_BOX_AP_THRS 10         /* IoU thresholds of stl_box_ap_match (.50:.05:.95) */
#define STL_BOX_AP_AREAS 4         /* area ranges of stl_box_ap_match (all, small, medium, large) */
#define STL_BOX_AP_DETS 100        /* detections kept per (image, category): the largest maxDets */
#define STL_BOX_AP_GT_MAX 128      /* ground truths per (image, category): the fp64 IoU tile [100, 128] is 100 KiB of LDS at the cap */
#define STL_BOX_AP_SCAN_TILE 1024  /* slots per scan step of stl_box_ap_accumulate (its workgroup size) */
#define STL_BOX_AP_MAXDETS_MAX 8   /* maxDets values of one stl_box_ap_accumulate call */
#define STL_BOX_AP_RECS_MAX 101    /* recall points of one stl_box_ap_accumulate call */

/* COCOeval.evaluateImg for "bbox", one workgroup per (image, category).  Detections: boxes fp64 [N, 4] (x, y, w, h), scores fp32
 * [N] (no NaN), labels int64 [N], det_offsets int64 [I + 1] (image i owns rows det_offsets[i] .. det_offsets[i+1]-1, at most max_n
 * <= STL_BOX_MAX of them).  Ground truth: gt_boxes fp64 [G, 4] (x, y, w, h), gt_area fp64 [G], gt_label int64 [G], gt_crowd uint8
 * [G], gt_offsets int64 [I + 1]; at most max_g <= STL_BOX_AP_GT_MAX rows per (image, category).  cats int64 [K], strictly
 * ascending.  All of these are device pointers.  iou_thrs [STL_BOX_AP_THRS] and area_ranges [STL_BOX_AP_AREAS][2] (lo, hi) are
 * HOST arrays of doubles: they travel in the kernel arguments.
 * Per (image, category): the detections with that label in stable descending score order (ties keep input order), the first
 * STL_BOX_AP_DETS kept; iou = maskApi.bbIou in fp64 (w = min(dx+dw, gx+gw) - max(dx, gx), <= 0 gives 0, the same for h; i = w*h;
 * u = crowd ? dw*dh : dw*dh + gw*gh - i; i / u); per threshold t and area range the greedy match in score order: best = min(t,
 * 1 - 1e-10), walk the ground truth (non-ignored first, stable; ignored = crowd or area < lo or area > hi), skip a matched
 * non-crowd one, stop at the first ignored one once a non-ignored one is held, skip iou < best, else take it (a tie moves to the
 * later one).  A matched detection inherits its match's ignore flag; an unmatched one is ignored when its w*h is outside the range.
 * Outputs, one slot per detection row (the caller presets slot_cat to -1: rows whose label is not in cats, or beyond the first
 * STL_BOX_AP_DETS of their category, keep it): the kept detections of (image i, category k) fill the slots det_offsets[i] + (rows
 * of the image with a smaller label) + rank, rank = 0 .. in score order, with slot_score, slot_cat = k, slot_rank = rank and bit
 * t * STL_BOX_AP_AREAS + a of slot_matched / slot_ignored.  npig int32 [I, K, STL_BOX_AP_AREAS]: the non-ignored ground truths
 * (-1: the segment was refused, its offsets are inconsistent or above the caps). */
int stl_box_ap_match(const double* boxes, const float* scores, const int64_t* labels, const int64_t* det_offsets, int64_t N, int max_n,
                     const double* gt_boxes, const double* gt_area, const int64_t* gt_label, const uint8_t* gt_crowd,
                     const int64_t* gt_offsets, int64_t G, int max_g, int num_images, const int64_t* cats, int K,
                     const double* iou_thrs, const double* area_ranges, float* slot_score, int32_t* slot_cat, int32_t* slot_rank,
                     uint64_t* slot_matched, uint64_t* slot_ignored, int32_t* npig, void* stream);
/* COCOeval.accumulate with the reductions of summarize, one workgroup per (threshold, area range, maxDets, category); it knows
 * nothing of boxes.  matched / ignored uint64 [S] (bit t * A + a), rank int32 [S]; order int64 [S]: the slots grouped by category,
 * each group in stable descending score order (images ascending, ranks ascending among equal scores); cat_offsets int64 [K + 1]:
 * category k owns order[cat_offsets[k] .. cat_offsets[k+1]-1]; npig int64 [K, A]: non-ignored ground truths over all images.
 * max_dets [M] and rec_thrs [R] (rising from 0) are HOST arrays.  Over the group's slots with rank < max_dets[m]: tp = prefix count
 * of matched & !ignored, fp = of !matched & !ignored, rc = tp / npig, pr = tp / (fp + tp + 2^-52) in fp64;
 * recall fp64 [T, K, A, M] = the last rc (0 without slots); precision fp64 [T, R, K, A, M] = per recall point r the largest pr
 * over the positions with rc >= r (0 if none): the precision envelope read at searchsorted(rc, r, "left").  npig == 0: -1. */
int stl_box_ap_accumulate(const uint64_t* matched, const uint64_t* ignored, const int32_t* rank, const int64_t* order,
                          const int64_t* cat_offsets, const int64_t* npig, int64_t S, int K, int T, int A, const int32_t* max_dets,
                          int M, const double* rec_thrs, int R, double* precision, double* recall, void* stream);

/* ---- Pose scoring (stlpose_amd/csrc/keypoint_eval.hip, coco_match.inc): the tail of src/03_evaluate.py, i.e. rescoring + OKS-NMS
 * (lib/metrics.py:211-262, lib/nms.py) and the published COCOeval(..., "keypoints").evaluateImg; the accumulate step above
 * finishes keypoint AP unchanged (T = 10, A = 3).  17 joints.  Exact up to exp: every operation is fp64 as written in that file's
 * head; the device's fp64 exp and the sum of at most 17 terms may differ from numpy's in the last bits (one OKS by less than
 * 1e-13), and OKS values are only compared, so the outputs equal the host's whenever no comparison is closer than that. */
#define STL_POSE_JOINTS 17         /* joints of a pose in this section */
#define STL_POSE_NMS_MAX 1024      /* persons per image of the rescoring + NMS entry point */
#define STL_POSE_SUM_NUMPY 0       /* sum_order of the rescoring: numpy's pairwise order */
#define STL_POSE_SUM_SERIAL 1      /* ... one running sum, the reference's loop */
#define STL_OKS_AP_THRS 10         /* OKS thresholds of the match (.50:.05:.95) */
#define STL_OKS_AP_AREAS 3         /* area ranges of the match (all, medium, large) */
#define STL_OKS_AP_DETS 20         /* detections kept per image: the largest maxDets */

/* Rescoring and greedy OKS suppression over a ragged table, one workgroup per image.  preds [P, 17, 3] (x, y, confidence) of
 * fp32 (preds_f64 = 0) or fp64 (1), boxes fp64 [P, 6] (centre x, y, scale x, y, area, box score), offsets int64 [I + 1]: image i
 * owns rows offsets[i] .. offsets[i+1]-1, at most max_n <= STL_POSE_NMS_MAX of them (an image above max_n gets count -1).
 * score fp64 [P] = box score x mean confidence of the joints with confidence > in_vis_thr (compared in the dtype of preds), 0 if
 * there is none; the mean in that dtype, divided by n, the product in fp64.  sum_order STL_POSE_SUM_NUMPY: numpy's order, what
 * conf[good].mean() of the host function gives (n < 8: a running sum; else eight running sums over the first 8 * (n / 8)
 * values, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the rest in order); STL_POSE_SUM_SERIAL: one running sum over the joints
 * in order, what the reference's loop gives (lib/metrics.py:242-250).  The two differ by an ulp for some n >= 8.
 * Suppression: descending score, equal scores in descending input position; a candidate goes when its OKS with a kept person
 * exceeds oks_thr.  OKS = sum_k exp(-e_k) / 17, e_k = (dx^2 + dy^2) / var[k] / ((area_kept + area_cand) / 2 + 2^-52) / 2, fp64,
 * var [17] a HOST array ((2 sigma)^2).  keep int32 [P]: per image segment the image-local rows of the kept persons in that
 * order, then -1; count int32 [I]. */
int stl_pose_rescore_nms(const void* preds, int preds_f64, int sum_order, const double* boxes, const int64_t* offsets, int num_images, int64_t P,
                         int max_n, double in_vis_thr, double oks_thr, const double* var, double* score, int32_t* keep,
                         int32_t* count, void* stream);
/* COCOeval.evaluateImg for "keypoints", one workgroup per image.  Detections: kpts fp64 [N, 17, 3], scores fp64 [N] (no NaN), area
 * fp64 [N] or NULL (then (max x - min x) * (max y - min y) over the 17 joints), det_offsets int64 [I + 1], at most max_n <=
 * STL_BOX_MAX rows per image.  Ground truth: gt_kpts fp64 [G, 17, 3] (x, y, visibility), gt_area fp64 [G], gt_bbox fp64 [G, 4]
 * (x, y, w, h), gt_crowd uint8 [G], gt_numkp int32 [G], gt_offsets int64 [I + 1], at most max_g <= STL_BOX_AP_GT_MAX rows per
 * image.  oks_thrs [STL_OKS_AP_THRS], area_ranges [STL_OKS_AP_AREAS][2] (lo, hi, both inclusive) and var [17] are HOST arrays.
 * Per image: the detections in stable descending score order (-0 == +0), the first STL_OKS_AP_DETS kept; the ground truth per
 * area range with the ignored last, stable (ignored: crowd, or gt_numkp == 0, or area outside the range); OKS as computeOks
 * writes it: over the joints with visibility > 0 when there is one (dx = xd - xg), else over all 17 with the distance to the
 * doubled box (dx = max(0, x0 - xd) + max(0, xd - x1), x0 = x - w, x1 = x + 2 w); e = (dx^2 + dy^2) / var / (gt_area + 2^-52) / 2,
 * the mean of exp(-e).  The greedy match is that of the box match above with OKS for IoU (a crowd can be matched again; an
 * unmatched detection whose area is outside the range is ignored).  Outputs as there with K = 1: the kept detections of image i
 * fill the slots det_offsets[i] + rank with slot_score (fp64), slot_cat = 0 (the caller presets -1), slot_rank and bit
 * t * STL_OKS_AP_AREAS + a of slot_matched / slot_ignored; npig int32 [I, 1, STL_OKS_AP_AREAS] (-1: the image was refused). */
int stl_oks_ap_match(const double* kpts, const double* scores, const double* area, const int64_t* det_offsets, int64_t N, int max_n,
                     const double* gt_kpts, const double* gt_area, const double* gt_bbox, const uint8_t* gt_crowd,
                     const int32_t* gt_numkp, const int64_t* gt_offsets, int64_t G, int max_g, int num_images,
                     const double* oks_thrs, const double* area_ranges, const double* var, double* slot_score, int32_t* slot_cat,
                     int32_t* slot_rank, uint64_t* slot_matched, uint64_t* slot_ignored, int32_t* npig, void* stream);

/* ---- EfficientDet person detector (stlpose_amd/csrc/detector.hip): src/models/EfficientDet.py with
 * models/efficientdet_utils/{model,utils}.py and models/efficientnet/{model,utils,utils_extra}.py, NHWC activations; inference, and
 * fine-tuning of the heads (further down).
 * The stl_det_* entry points without a suffix are the fp32 path.  The *16 entry points further down are the 16-bit compute modes
 * (EfficientDetBackbone(compute_dtype="bf16" | "f16")): activations stored as STL_BF16 or STL_F16, every sum in fp32. */
#define STL_DET_NMS_MAX 65536      /* candidates per image of stl_det_nms (all 49104 anchors of a 512 canvas fit) */

/* One source image of stl_det_preprocess.  kind 0: uint8 HWC RGB (divided by 255), 1: float CHW in [0, 1]; new_h / new_w from
 * aspectaware_resize_padding (efficientdet_utils/utils.py:209-239, computed on the host); scale_* = old / new (cv2's 1 / inv_scale). */
typedef struct {
    const void* src;
    int32_t kind, old_h, old_w, new_h, new_w, pad_;
    double scale_y, scale_x;
} StlDetImage;

/* preprocess (efficientdet_utils/utils.py:190-207): transforms.Normalize(mean (0.406, 0.456, 0.485), std (0.225, 0.224, 0.229)),
 * cv2.resize INTER_LINEAR to new_h x new_w (half-pixel centres, clamped source, no antialias; a copy at the identity size), zero
 * S x S canvas with the image at the top left.  imgs: B records in device memory; out fp32 [B, S, S, 3]. */
int stl_det_preprocess(const StlDetImage* imgs, int B, int S, float* out, void* stream);
/* _conv_stem + _bn0 + swish (efficientnet/model.py:151-153, efficientdet_utils/model.py:405-407): 3 -> Co 3x3 s2, TF same padding
 * (utils_extra.py:37-50), BN folded into w [3][3][3][Co] and bias [Co].  x [B, H, W, 3] -> out [B, ceil(H/2), ceil(W/2), Co]. */
int stl_det_stem(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int Co, void* stream);
/* Depthwise k x k (k 3 or 5) stride s (1 or 2) conv with TF same padding (MBConvBlock._depthwise_conv + _bn1 + swish,
 * efficientnet/model.py:80-82; SeparableConvBlock.depthwise_conv, efficientdet_utils/model.py:40).  w [k][k][C] (BN scale folded),
 * bias [C] or NULL, act 1: swish.  x [B, H, W, C] -> out [B, ceil(H/s), ceil(W/s), C]. */
int stl_det_dwconv(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C, int k, int s, int act,
                   void* stream);
/* Squeeze-excitation (efficientnet/model.py:84-89): scale [B, C] = sigmoid(w2 swish(w1 mean_hw(x) + b1) + b2), w1 [Cs][C],
 * w2 [C][Cs].  partial: stl_det_se_workspace(B) * C floats; the per-channel sums are taken in a fixed order. */
int stl_det_se(const float* x, int B, int HW, int C, int Cs, const float* w1, const float* b1, const float* w2, const float* b2,
               float* partial, float* scale, void* stream);
int stl_det_se_workspace(int B);

/* 1x1 conv as a GEMM on v_mfma_f32_16x16x4_f32: out[img(m) * out_img_stride + pix(m) * out_row_stride + out_off + n] =
 * act(sum_k x[m, k] * in_scale[img(m), k] * w[k, n] + bias[n]) + residual[m, n], m < M = B * HW.  x [M, Ci] (any Ci), w packed
 * [Kp][Np] zero-padded (Kp % 16 == 0, Np % 64 == 0), bias [>= Co] or NULL, in_scale [B, Ci] or NULL (the SE scale applied on
 * load), residual [M, Co] or NULL, act 0 none / 1 swish / 2 sigmoid (after the bias, before the residual). */
typedef struct {
    const float* x;
    const float* w;
    const float* bias;
    const float* in_scale;
    const float* residual;
    float* out;
    int64_t M, out_img_stride, out_row_stride, out_off;
    int32_t HW, Ci, Co, Kp, Np, act;
} StlDetPointwise;
int stl_det_pointwise(const StlDetPointwise* p, void* stream);

/* One BiFPN input: x [B, H, W, C] read as mode 0 the same size, 1 nearest 2x upsample (nn.Upsample(scale_factor=2)), 2 the 3x3 s2
 * max-pool of MaxPool2dStaticSamePadding (TF same padding, padded with zeros by F.pad before the max, utils_extra.py:80-86). */
typedef struct {
    const float* x;
    int32_t mode, H, W, pad_;
} StlDetTerm;
/* BiFPN node input (efficientdet_utils/model.py:163-233): out [B, H, W, C] = swish(sum_i w_i * read(t_i)), w = relu(wparam) /
 * (sum relu(wparam) + 1e-4) normalised on the device from the nterms raw parameters, summed left to right.  wparam NULL (one
 * term): out = read(t_0), the pooled maps of p5_to_p6 / p6_to_p7. */
typedef struct {
    int32_t B, H, W, C, nterms, pad_;
    StlDetTerm t[3];
    const float* wparam;
    float* out;
} StlDetFuse;
int stl_det_fuse(const StlDetFuse* f, void* stream);

/* -- 16-bit compute modes.  dtype is STL_BF16 or STL_F16 (anything else is an error).  Every 16-bit tensor is NHWC with C % 8 == 0
 * (true of every tensor the network stores: the B0 / B3 widths and expansions, BiFPN 64 / 160): one 16-byte access moves 8 channels,
 * and any other C is an error ("... C % 8 == 0" in stl_last_error) before anything is launched.  Tensors and the fp32 weight,
 * bias and scale arrays must be 16-byte aligned.  Sums, depthwise weights, biases, the SE and attention arithmetic are fp32; a value is
 * rounded to dtype once, when it is stored.  f16 activations past 65504 become inf: the model's f16 mode checks its head outputs. */
/* stl_det_stem with a dtype output: x fp32 [B, H, W, 3] -> out dtype [B, ceil(H/2), ceil(W/2), Co]. */
int stl_det_stem16(int dtype, const float* x, const float* w, const float* bias, void* out, int B, int H, int W, int Co, void* stream);
/* stl_det_dwconv on dtype tensors, w [k][k][C] and bias [C] (or NULL) fp32, 8 channels per thread.  partial non-NULL (the MBConv
 * case): also writes the squeeze-excitation pooling sums partial[B][stl_det_dw16_parts(Ho * Wo)][C], one slot per workgroup of
 * pixels: the sum of that workgroup's fp32 outputs before rounding, added in a fixed order (no atomics); every slot is written. */
int stl_det_dwconv16(int dtype, const void* x, const float* w, const float* bias, void* out, float* partial, int B, int H, int W, int C,
                     int k, int s, int act, void* stream);
int stl_det_dw16_parts(int HoWo);
/* stl_det_se from pooling sums: partial [B][nparts][C] is added in slot order and divided by HW; scale fp32 [B, C] as stl_det_se. */
int stl_det_se16(const float* partial, int B, int HW, int nparts, int C, int Cs, const float* w1, const float* b1, const float* w2,
                 const float* b2, float* scale, void* stream);
/* stl_det_pointwise on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation.  x dtype [M, Ci], Ci % 8 == 0.  w dtype, packed
 * [Np / 16][Kp / 32][64][8]: element ((nt * (Kp / 32) + ks) * 64 + 16 * g + r) * 8 + i is w[k = 32 ks + 8 g + i][n = 16 nt + r],
 * zero-padded to Kp % 32 == 0, Np % 64 == 0.  bias fp32 [Np] or NULL.  in_scale fp32 [B, Ci] or NULL: x * in_scale in fp32, rounded
 * once to dtype.  residual dtype [M, Co] or NULL.  out_f32 0: out dtype (Co, strides and offset multiples of 4: the 4 channels a
 * lane holds are one 8-byte store); out_f32 1: out fp32 with any Co, strides and offset (the head headers writing into reg / cls).
 * MI355X, batch 32: the 16-bit forward takes 5.2 ms (D0) / 11.7 ms (D3) against 14.3 / 34.2 ms in fp32 (profiles/detector_bench.json). */
typedef struct {
    const void* x;
    const void* w;
    const float* bias;
    const float* in_scale;
    const void* residual;
    void* out;
    int64_t M, out_img_stride, out_row_stride, out_off;
    int32_t HW, Ci, Co, Kp, Np, act, dtype, out_f32;
} StlDetPointwise16;
int stl_det_pointwise16(const StlDetPointwise16* p, void* stream);
/* stl_det_fuse on dtype tensors (t[i].x and out point at dtype elements), the attention weights fp32, 8 channels per thread. */
int stl_det_fuse16(const StlDetFuse* f, int dtype, void* stream);

/* postprocess up to the NMS (efficientdet_utils/utils.py:14-56, 150-168): per image, score = max over the nc classes (first
 * maximum), kept when score > thr; BBoxTransform (exp) on anchors fp32 [A][4] (y1, x1, y2, x2) and reg [B, A, 4] (dy, dx, dh, dw);
 * ClipBoxes to [0, xmax] x [0, ymax].  The survivors in anchor order: boxes [B, A, 4] (x1, y1, x2, y2), scores [B, A], classes
 * [B, A], index [B, A] (the anchor), the first count[b] rows of image b.  One workgroup per image. */
int stl_det_decode(const float* reg, const float* cls, const float* anchors, int B, int A, int nc, float thr, float xmax, float ymax,
                   float* boxes, float* scores, int32_t* classes, int32_t* index, int32_t* count, void* stream);
/* torchvision.ops.batched_nms as torchvision 0.4 runs it (postprocess, efficientdet_utils/utils.py:169): boxes [n, 4] offset by
 * class * (max coordinate + 1), then nms in the given order (order int32 [n]: descending score, ties to the lower index) -- a
 * 64 x 64 bitmask IoU matrix and a one-wave greedy sweep, so any n <= STL_DET_NMS_MAX.  keep int32 [n]: the first count kept
 * candidate indices in score order.  work: stl_det_nms_workspace(n) bytes. */
int stl_det_nms(const float* boxes, const int32_t* classes, const int32_t* order, int n, double iou_thr, void* work, int32_t* keep,
                int32_t* count, void* stream);
int64_t stl_det_nms_workspace(int n);

/* -- Fine-tuning the heads (stlpose_amd/csrc/detector_train.hip; stlpose_amd/detector_train.py).  The backbone and the BiFPN are
 * frozen and every BN runs on its running statistics, so the heads are depthwise 3x3 -> pointwise (bias and BN folded, W' and b')
 * -> swish per layer and level, and a header.  fp32, NHWC; every reduction in a fixed order (two runs are bitwise equal). */
/* stl_det_pointwise with act 1 (swish) and no residual that also keeps the pre-activation: z [M, Co] = x w + bias, out = swish(z).
 * The kernel of stl_det_pointwise: out equals that call's bit for bit. */
int stl_det_pointwise_train(const StlDetPointwise* p, float* z, void* stream);
/* The RetinaNet / EfficientDet detection loss (no reference item; restated in tests/detector_train_ref.py).  reg [B, A, 4] (dy, dx,
 * dh, dw), cls [B, A, nc] after the sigmoid, anchors [A, 4] (y1, x1, y2, x2), gt [sum G, 5] (x1, y1, x2, y2, class) on the canvas with
 * offsets int32 [B + 1] (gt may be NULL when every image is empty).  Per image: IoU = inter / max(area_a + area_g - inter, 1e-8); an
 * anchor is positive (first argmax g*) at max IoU >= 0.5, negative below 0.4, ignored between, negative when the image has no box.
 * Classification, p = clamp(cls, 1e-4, 1 - 1e-4): alpha (1 - p)^gamma (-log p) at (positive, class of g*), (1 - alpha) p^gamma
 * (-log(1 - p)) at every other class of a positive or negative anchor, summed and divided by max(N_pos, 1).  Regression over the
 * positives: smooth L1 (4.5 d^2 if d <= 1/9, else d - 1/18) of d = |t - reg|, t = ((cy_g - cy_a) / h_a, (cx_g - cx_a) / w_a,
 * log(h_g / h_a), log(w_g / w_a)) with w_g, h_g >= 1, mean over 4 N_pos (0 without positives).  losses [2] = (mean_b L_cls,b,
 * box_weight * mean_b L_reg,b); dreg [B, A, 4] and dlogit [B, A, nc] are the gradients of losses[1] and losses[0] with respect to
 * reg and to the classifier header's pre-sigmoid output (zero where the clamp is active); npos int32 [B].  Workspaces: assign int32
 * [B, A], per_image [B, 2].  One workgroup per image (N_pos normalises that image's gradients), then one launch for the batch means. */
int stl_det_loss(const float* reg, const float* cls, const float* anchors, const float* gt, const int32_t* offsets, int B, int A, int nc,
                 float alpha, float gamma, float box_weight, int32_t* assign, float* per_image, float* losses, float* dreg, float* dlogit,
                 int32_t* npos, void* stream);
/* Backward of stl_det_pointwise (no in_scale, no residual; the activation's derivative is already in dy).  dy is read as the forward
 * writes its output: dy[img(m) * dy_img_stride + pix(m) * dy_row_stride + dy_off + n], so a header's gradient comes straight out of
 * the concatenated [B, A, k] tensor.  w is the forward's packed [Kp][Np].
 *   bwd_data:   dx [M, Ci] = sum_n dy[m, n] w[k, n]                                       (reads w, dy; writes dx)
 *   bwd_weight: dw [Ci][Co] = sum_m x[m, k] dy[m, n], db [Co] = sum_m dy[m, n]            (reads x [M, Ci], dy; writes dw, db)
 * bwd_weight splits M into stl_det_pointwise_bwd_slabs(M) slabs over workgroups and adds them in slab order; partial holds
 * slabs * (Ci * Co + Co) floats.  Both run on v_mfma_f32_16x16x4_f32. */
typedef struct {
    const float* x;
    const float* w;
    const float* dy;
    float* dx;
    float* dw;
    float* db;
    float* partial;
    int64_t M, dy_img_stride, dy_row_stride, dy_off;
    int32_t HW, Ci, Co, Kp, Np, pad_;
} StlDetPointwiseBwd;
int stl_det_pointwise_bwd_data(const StlDetPointwiseBwd* p, void* stream);
int stl_det_pointwise_bwd_weight(const StlDetPointwiseBwd* p, void* stream);
int stl_det_pointwise_bwd_slabs(int64_t M);
/* Backward of stl_det_dwconv with k 3, s 1, no bias, no activation (the heads' depthwise layers).  bwd_data: dx [B, H, W, C] =
 * sum_{ky, kx} dy[b, y + 1 - ky, x + 1 - kx, c] w[ky][kx][c] (w as the forward takes it; the kernel flips the taps), times swish'(z)
 * when z [B, H, W, C] (the stored pre-activation of the layer below) is not NULL.  bwd_weight: dw [3][3][C] = sum over batch and
 * pixels of x[b, y - 1 + ky, x - 1 + kx, c] dy[b, y, x, c]: stl_det_dwconv_bwd_parts(B * H * W) partial sums (partial: parts * 9 * C
 * floats), then added in part order. */
int stl_det_dwconv_bwd_data(const float* dy, const float* w, const float* z, float* dx, int B, int H, int W, int C, void* stream);
int stl_det_dwconv_bwd_weight(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, int C, void* stream);
int stl_det_dwconv_bwd_parts(int64_t npix);

/* -- Fine-tuning the heads of a 16-bit model (EfficientDetBackbone(compute_dtype="f16").detection_loss): f16 forward, bf16 gradients,
 * the recipe of the pose network's mixed mode.  The arithmetic contract, which tests/detector_train16_ref.py emulates:
 *   forward   exactly the 16-bit inference plan: the depthwise output d, the swish output t and the kept pre-activation z are stored
 *             in dtype, each rounded once from its fp32 value (t = round(swish(z_fp32)), so reg / cls equal inference bit for bit);
 *             reg, cls, stl_det_loss and its dreg / dlogit stay fp32.
 *   backward  gradients in flight are bf16, rounded once when stored.  Pointwise data gradient dX = dY W'^T: dY bf16 (a header's
 *             fp32 dreg / dlogit is rounded to bf16 in registers), W'^T from a bf16 pack rounded once from the same fp64 fold as the
 *             forward pack, fp32 accumulation, dX stored bf16.  Pointwise weight gradient dW' = X^T dY, db' = sum dY: X is the stored
 *             dtype tensor converted to bf16 while staging, dY bf16 (db' adds the same bf16 values the MFMA sees), fp32 sums, dW' and
 *             db' stored fp32.  Depthwise: taps fp32, fp32 VALU arithmetic, dY bf16, swish'(z) in fp32 from the stored z, dX stored
 *             bf16; the weight gradient multiplies x (dtype) and dY (bf16) in fp32, fp32 partial sums, dw fp32.
 * Every reduction in a fixed order, no atomics: two runs are bitwise equal.  16-bit tensors need C % 8 == 0 and 16-byte alignment as
 * above; a failed check sets stl_last_error and launches nothing.
 * tools/detector_train_bench.py times the f16 step, its trunk and the heads' share next to the fp32 ones in one run and fails if the
 * f16 step is not faster than fp32 at batch 32 (profiles/detector_train_bench.json).  Step fp32 -> f16 at batch 32: D0 30.5 -> 20.0 ms,
 * D3 59.6 -> 30.0 ms; trunk 12.8 -> 4.5 and 29.4 -> 10.0 ms; heads' share (with the f16 step's host wait for the non-finite check)
 * 17.7 -> 15.5 and 30.2 -> 20.0 ms.  At batch 8: D3 30.4 -> 22.2 ms (heads 17.6 -> 16.6); D0 16.4 -> 14.2 ms with a heads' share
 * that is not below fp32's (10.9 -> 11.8 ms): short kernels, the same 150 launches, and per step a refold of the transposed packs
 * on the host and one wait for the device. */
/* stl_det_pointwise16 with act 1 (swish), no residual and a 16-bit output that also keeps the pre-activation: z dtype [M, Co] =
 * round(x w + bias), out = round(swish(x w + bias)).  The kernel of stl_det_pointwise16: out equals that call's bit for bit. */
int stl_det_pointwise16_train(const StlDetPointwise16* p, void* z, void* stream);
/* Backward of stl_det_pointwise16 (no in_scale, no residual; the activation's derivative is already in dy), both on
 * v_mfma_f32_16x16x32_bf16.  x xdtype (STL_F16 or STL_BF16) [M, Ci], Ci % 8 == 0.  dy is addressed as in StlDetPointwiseBwd:
 * dy_f32 0: bf16, Co, strides and offset multiples of 8 (16-byte loads); dy_f32 1: the strided fp32 [B, A, k] tensor of a header,
 * any Co, rounded to bf16 in registers.  wt is the bf16 transposed pack: the forward's layout with the roles of k and n swapped,
 * [Np / 16][Kp / 32][64][8] with element ((kt * (Kp / 32) + ns) * 64 + 16 * g + r) * 8 + i = W'[k = 16 kt + r][n = 32 ns + 8 g + i],
 * zero-padded to Kp = ceil(Co / 32) * 32 and Np = ceil(Ci / 64) * 64.
 *   bwd_data:   dx bf16 [M, Ci] = sum_n dy[m, n] W'[k, n]; dY rows are read straight from global memory, 8 consecutive n per lane
 *   bwd_weight: dw fp32 [Ci][Co] = sum_m x[m, k] dy[m, n], db fp32 [Co] = sum_m dy[m, n]: the contraction runs over m, so 64-row
 *               tiles of x and dy are staged through LDS transposed (two rows paired in registers, dword writes, 16-byte reads)
 * Rows past M and channels past Ci / Co contribute exact zeros and are never read.  bwd_weight splits M into
 * stl_det_pointwise16_bwd_slabs(M) slabs and adds them in slab order; partial holds slabs * (Ci * Co + Co) floats. */
typedef struct {
    const void* x;
    const void* wt;
    const void* dy;
    void* dx;
    float* dw;
    float* db;
    float* partial;
    int64_t M, dy_img_stride, dy_row_stride, dy_off;
    int32_t HW, Ci, Co, Kp, Np, xdtype, dy_f32, pad_;
} StlDetPointwise16Bwd;
int stl_det_pointwise16_bwd_data(const StlDetPointwise16Bwd* p, void* stream);
int stl_det_pointwise16_bwd_weight(const StlDetPointwise16Bwd* p, void* stream);
int stl_det_pointwise16_bwd_slabs(int64_t M);
/* Backward of stl_det_dwconv16 with k 3, s 1, no bias, no activation, 8 channels per thread and 16-byte accesses (C % 8 == 0).
 * bwd_data: dy bf16, w fp32 [3][3][C], z zdtype [B, H, W, C] or NULL, dx bf16 = (flipped-tap sum in fp32) * swish'(z).  bwd_weight:
 * x xdtype, dy bf16, dw fp32 [3][3][C] through stl_det_dwconv16_bwd_parts(B * H * W) fp32 partial sums (partial: parts * 9 * C
 * floats) added in part order. */
int stl_det_dwconv16_bwd_data(const void* dy, const float* w, const void* z, void* dx, int B, int H, int W, int C, int zdtype, void* stream);
int stl_det_dwconv16_bwd_weight(int xdtype, const void* x, const void* dy, float* partial, float* dw, int B, int H, int W, int C,
                                void* stream);
int stl_det_dwconv16_bwd_parts(int64_t npix);

/* ---- AdaIN feed-forward stylisation (csrc/adain.hip; stlpose_amd/adain.py).  No reference counterpart: the network is the published
 * one (Huang & Belongie 2017), restated in tests/adain_ref.py.  The 3x3 convs pad by reflection and stl_conv pads with zeros, so every
 * conv runs as a "same" conv on an explicitly padded (H+2) x (W+2) NHWC map whose output ring is never read.  dtype STL_F32 or STL_BF16
 * throughout; element indices are 32-bit (every tensor below 2^31 elements). */
#define STL_GATHER_COPY 0
#define STL_GATHER_UP 1   /* nn.Upsample(scale_factor=2, mode="nearest") */
#define STL_GATHER_POOL 2 /* nn.MaxPool2d(2, 2), floor */
/* img NCHW fp32 [B,3,H,W] -> out [B,H,W,32]: out[b,y,x,(ky*3+kx)*3+c] = img[b,c,reflect(y+ky-1,H),reflect(x+kx-1,W)], 0 for k >= 27
 * (stl_patch3x3's column order, so conv1_1 is the same 1x1 conv with Ci = 32; no ring: every tap is a real pixel). */
int stl_adain_input(int dtype, const float* img, void* out, int B, int H, int W, void* stream);
/* Padded input of the next conv from the interior of the previous output.  src [B, Hs+2*ring, Ws+2*ring, C] whose interior Hs x Ws
 * starts at (ring, ring), ring 0 or 1; v = op(src interior) is H x W = Hs x Ws (copy), 2Hs x 2Ws (up) or Hs/2 x Ws/2 (pool);
 * out [B, H+2, W+2, C]: out[b,y,x,c] = v[b, reflect(y-1,H), reflect(x-1,W), c].  scale / offset fp32 [B,C] or both NULL: every
 * loaded value becomes x * scale[b,c] + offset[b,c] (a multiply, then an add) before the op.  C % 8 == 0; H, W >= 2. */
int stl_reflect_gather(int dtype, const void* src, void* out, int B, int Hs, int Ws, int ring, int C, int op, const float* scale,
                       const float* offset, void* stream);
/* Per (image, channel) statistics over the interior H x W of x [B, H+2*ring, W+2*ring, C]: mean, unbiased variance and
 * sigma = sqrt(var + eps), each fp32 [B,C].  Sums and sums of squares in fp64, added in a fixed order (deterministic).
 * partial: workspace of B * nchunk * 2 * C doubles; nchunk >= 1 workgroups share an image's pixels. */
int stl_adain_stats(int dtype, const void* x, int B, int H, int W, int ring, int C, int nchunk, double* partial, float eps, float* mean,
                    float* var, float* sigma, void* stream);
/* AdaIN and the alpha blend as one affine of the content features: with m_s = sum_k weights[b,k] * mean_s[k,c] and s_s likewise from
 * sigma_s (fp32 [S,C]; weights fp32 [B,S]), r = s_s / sqrt(var_c + eps): scale = alpha * r + (1 - alpha),
 * offset = alpha * (m_s - mean_c * r), fp32 [B,C].  fp64 inside; alpha = 0 gives exactly (1, 0). */
int stl_adain_affine(const float* mean_c, const float* var_c, const float* mean_s, const float* sigma_s, const float* weights, int B, int C,
                     int S, float alpha, float eps, float* scale, float* offset, void* stream);
/* Interior of the last conv's output x [B, H+2, W+2, C] (C = its Co padded to 8), channels 0..2 -> out NCHW fp32 [B,3,H,W];
 * clamp != 0: to [0, 1]. */
int stl_adain_output(int dtype, const void* x, float* out, int B, int H, int W, int C, int clamp, void* stream);

const char* stl_last_error(void);
int stl_version(void);
/* Hash (16 hex digits) of the kernel and header sources this library was compiled from (stlpose_amd/build.py). */
const char* stl_build_id(void);
/* Name of the kernel instantiation the calling thread launched last, e.g. "conv_core_kernel<bf16,3,4,2,4,2,3,1,0,1,-1,0>"
 * (template arguments in declaration order) -- measurement only: bench.py groups per-launch timings by it. */
const char* stl_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
