/*
 * stlpose_hip_det_batch.h -- detector training / validation batches built on the device (stlpose_amd/csrc/det_batch.hip): from
 * resident uint8 images and the annotation tables of stlpose_amd/det_data.py to the network's canvas and the ground-truth table
 * stl_det_loss reads, in ONE launch per batch.  Part of libstlpose_hip.so; written in the C subset of stlpose_hip.h and read by the
 * same reader (stlpose_amd/capi.py).
 */
#ifndef STLPOSE_HIP_DET_BATCH_H
#define STLPOSE_HIP_DET_BATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define STL_DET_BATCH_MAX 1024     /* images per launch of stl_det_batch (the offset scan is one workgroup's) */
#define STL_DET_BATCH_SIDE 4096    /* largest S1 and S (stl_det_preprocess's cap) */

/* The chain ResizeImageDetection(S1) (data/custom_transforms.py:36-67) -> imgs / 255 -> stl_det_preprocess (Normalize + the
 * aspect-aware resize of the S1 x S1 square to the S x S canvas) without materialising anything in between, and the boxes through
 * the same two scalings.
 *
 * Inputs.  src: the uint8 HWC RGB image buffer of src_bytes bytes; src_off int64 [B] and src_hw int32 [B, 2] (height, width): where
 * each of the B chosen images lies (ResidentImages.rows).  index int64 [B]: the images' rows in the annotation tables box_start
 * int64 [N], box_count int32 [N], boxes fp32 [M, 4] (x1, y1, x2, y2 in source pixels), labels int64 [M] (1 = the first class).
 * draws: NULL, or one uniform fp64 draw per image; with flip_enabled an image whose draw is <= 0.5 is mirrored.
 *
 * Stage 1 (never stored unless asked for).  scale = S1 / max(h, w) in fp64; the longer side becomes S1 and the shorter
 * (int)(side * scale), the tie taking the reference's else branch (width = S1).  The rh x rw region is cv2.resize(INTER_LINEAR) as
 * this library states it (stl_det_preprocess: src = (dst + 0.5) * (1.0 / (new / old)) - 0.5 in fp64, rounded to fp32, floored,
 * clamped taps), the blend in fp32, horizontal then vertical, rounded to the nearest-even level; outside the region the square is 0.
 * cv2 blends uint8 images in 11-bit fixed point and can differ from this by one level: parity with cv2 is UNPINNED.
 * Mirrored: column x of the region reads what column rw - 1 - x would have been.
 * stage1: NULL, or uint8 [B, S1, S1, 3] that receives these images.
 *
 * (a) canvas fp32 [B, S, S, 3]: bit for bit what stl_det_preprocess writes for the stage-1 images as float CHW / 255.f (kind 1)
 *     with aspectaware_resize_padding's sizes of an S1 x S1 image on an S canvas.
 * (b) gt fp32 [gt_rows, 5] and offsets int32 [B + 1]: per box (x1, y1, x2, y2) * (float)scale in fp32 (mirrored: (rw - 1 - x2, y1,
 *     rw - 1 - x1, y2) in fp32), then times the fp64 ratio new / S1 of the canvas resize in fp64, rounded once to fp32; class =
 *     label - 1.  offsets: the exclusive scan of the chosen images' counts.  Rows from offsets[B] to gt_rows are zeroed; a row at or
 *     past gt_rows is not written (the caller sizes gt from the host table).
 * An index outside [0, N), or an image that does not lie inside the buffer, reads nothing: a zero canvas slice (and stage-1 image)
 * and no rows.  B <= STL_DET_BATCH_MAX, S1 and S <= STL_DET_BATCH_SIDE. */
int stl_det_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int32_t* src_hw, const int64_t* index,
                  const int64_t* box_start, const int32_t* box_count, int64_t N, const float* boxes, const int64_t* labels, int64_t M,
                  const double* draws, int flip_enabled, int B, int S1, int S, float* canvas, uint8_t* stage1, float* gt,
                  int64_t gt_rows, int32_t* offsets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
