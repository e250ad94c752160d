/*
 * stlpose_hip_detections.h -- the detector's device tail (stlpose_amd/csrc/detections.hip): from the head outputs to final
 * per-image detections and into a ragged store, without the host.  Part of libstlpose_hip.so; written in the C subset of
 * stlpose_hip.h, whose STL_BOX_MAX and StlDetImage it uses, and read by the same reader (stlpose_amd/capi.py).
 */
#ifndef STLPOSE_HIP_DETECTIONS_H
#define STLPOSE_HIP_DETECTIONS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* postprocess (efficientdet_utils/utils.py:150-187) and invert_affine (:242-256) in ONE launch, one 1024-thread workgroup per image
 * with its candidates in LDS (at most STL_BOX_MAX).  reg fp32 [B, A, 4] (dy, dx, dh, dw), cls fp32 [B, A, nc], anchors fp32 [A, 4]
 * (y1, x1, y2, x2).  Per image:
 *   1. the anchors whose best class score is > thr, in anchor order; the class is the first maximum;
 *   2. stable descending order by score (a bitonic sort of unique (score bits, position) keys);
 *   3. the boxes decoded with stl_det_decode's arithmetic, operation for operation (clamped to [0, xmax] x [0, ymax]);
 *   4. class-aware greedy NMS as stl_det_nms does it: every box shifted by class * (max coordinate over all the image's candidate
 *      boxes + 1) in fp32, iou = inter / (area_a + area_b - inter) left to right, a later box suppressed when (double)iou > iou_thr;
 *   5. images: NULL, or B StlDetImage records in device memory (those of stl_det_preprocess).  With them x is divided by
 *      (float)((double)new_w / old_w) and y by (float)((double)new_h / old_h): numpy's float32 array / Python float;
 *   6. the survivors in score order: boxes fp32 [B, K, 4] (x1, y1, x2, y2), scores fp32 [B, K], labels int32 [B, K] (class + 1),
 *      count int32 [B], with K = STL_BOX_MAX.  Rows past count are not written.
 * An image with n > STL_BOX_MAX candidates writes no row and gets count = -n - 1. */
int stl_det_postprocess(const float* reg, const float* cls, const float* anchors, const void* images, int B, int A, int nc,
                        float thr, float xmax, float ymax, double iou_thr, float* boxes, float* scores, int32_t* labels,
                        int32_t* count, void* stream);

/* One launch that moves a batch of stl_det_postprocess tables into a ragged store.  Store: st_boxes fp64 [cap, 4] (x, y, w, h with
 * w = x2 - x1 and h = y2 - y1 subtracted in fp32, then widened), st_scores fp32 [cap], st_labels int64 [cap]; slots int64 [*, 3]:
 * slot slot0 + i becomes (image_ids[i], start_i, count[i]) with start_i = cursor + the counts of the images before i (a negative
 * count adds no rows and is carried through unchanged).  cursor int64 [2] in device memory: the launch reads cursor[parity] and
 * writes cursor[1 - parity] = cursor[parity] + the batch's rows, so consecutive launches alternate parity.  A row at or past cap
 * is dropped and *overflow (int64) set to 1.  B <= 1024. */
int stl_det_append(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, const int64_t* image_ids,
                   int B, double* st_boxes, float* st_scores, int64_t* st_labels, int64_t cap, int64_t* slots, int64_t slot0,
                   int64_t* cursor, int parity, int64_t* overflow, void* stream);

/* The person rows of a batch of stl_det_postprocess tables for top-down pose extraction, on the device: bbox_filtering
 * (lib/bounding_box.py:127-168: labels == label and score > score_thr, in row order), then for iou_thr >= 0 stl_box_select's
 * torchvision NMS on the passing rows (score order), TransformDetection._coords2cs (lib/transforms.py:30-53) in fp32 as written, and
 * the crop -> image matrix of get_affine_transform(center, scale, 0, (crop_w, crop_h), inv=1) in closed form: r = scale_x * 200 /
 * crop_w, minv = (r, 0, cx - scale_x * 200 / 2; 0, r, cy - crop_h / 2 * r).  aspect: (float)(crop_w / crop_h).
 * Rows, adjacent and in image order, each table with room for B * STL_BOX_MAX rows: img int32 (the image's index in the batch),
 * out_boxes fp32 [*, 4], out_scores, center [*, 2], scale [*, 2], minv [*, 6]; total int32 [1]: the number of rows, or -(i) - 1
 * when image i carries a negative count (above the candidate cap).  1 launch without NMS, 3 with.  B <= 1024.
 * work: stl_person_boxes_workspace(B, iou_thr >= 0) bytes of device memory. */
int stl_person_boxes(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, int B, int label,
                     float score_thr, double iou_thr, float aspect, int crop_w, int crop_h, void* work, int32_t* img, float* out_boxes,
                     float* out_scores, float* center, float* scale, float* minv, int32_t* total, void* stream);
int64_t stl_person_boxes_workspace(int B, int nms);

#ifdef __cplusplus
}
#endif
#endif
