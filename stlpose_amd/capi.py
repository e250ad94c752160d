"""ctypes binding of libstlpose_hip.so (see include/stlpose_hip.h).

The product path has no CPU fallback: if the HIP library is missing this module raises at
import-of-symbols time (``lib()``), loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STLPOSE_HIP_LIB") or os.path.join(_HERE, "libstlpose_hip.so")   # override: A/B of two builds

F32, BF16, F16 = 0, 1, 2
DTYPES = {F32: (4, torch.float32), BF16: (2, torch.bfloat16), F16: (2, torch.float16)}   # code -> (bytes per element, torch dtype)


def dt2(grad_dtype: int, fwd_dtype: int) -> int:
    """STL_DT2: two element types in one int (low byte: gradient-side tensors, bits 8-15: forward-side tensors if different)."""
    return grad_dtype | ((fwd_dtype if fwd_dtype != grad_dtype else 0) << 8)


# pose retrieval (STL_POSE_* of include/stlpose_hip.h)
POSE_APPROACH = {"all_kpts": 0, "full_body": 1, "upper_body": 2}
POSE_DIM = {"all_kpts": 34, "full_body": 26, "upper_body": 18}
POSE_METHOD = {"euclidean": 0, "cosine": 1, "manhattan": 2, "confidence": 3, "oks": 4, "l2sq": 5, "cos_normalised": 6}
POSE_PEN = {"zero_coord": 0, "none": 1, "mean": 2, "max": 3}
POSE_TOPK_MAX, POSE_RANK_MAX, POSE_RANK_LABELS_MAX, POSE_NSCORES = 1024, 16384, 4, 10
POSE_RANK_ANY_MAX = 1 << 24   # STL_POSE_RANK_ANY_MAX: largest N of stl_pose_rank_any
# top-down extraction (STL_BOX_MAX, STL_RESIZE_SRC_MAX, STL_RESIZE_DST_MAX)
BOX_MAX, RESIZE_SRC_MAX, RESIZE_DST_MAX = 4096, 16384, 2048
# COCO box AP (STL_BOX_AP_*): thresholds, area ranges, detections kept per (image, category), ground truths per (image, category),
# scan tile, maxDets values and recall points per call
BOX_AP_THRS, BOX_AP_AREAS, BOX_AP_DETS, BOX_AP_GT_MAX, BOX_AP_SCAN_TILE, BOX_AP_MAXDETS_MAX, BOX_AP_RECS_MAX = 10, 4, 100, 128, 1024, 8, 101
# pose scoring (STL_POSE_JOINTS, STL_POSE_NMS_MAX, STL_OKS_AP_*): joints, persons per image of the NMS, OKS thresholds, area ranges,
# detections kept per image
POSE_JOINTS, POSE_NMS_MAX, OKS_AP_THRS, OKS_AP_AREAS, OKS_AP_DETS = 17, 1024, 10, 3, 20
POSE_SUM_ORDER = {"numpy": 0, "reference": 1}   # STL_POSE_SUM_NUMPY, STL_POSE_SUM_SERIAL
# person detector (STL_DET_NMS_MAX)
DET_NMS_MAX = 65536
# AdaIN gather ops (STL_GATHER_*)
GATHER_COPY, GATHER_UP, GATHER_POOL = 0, 1, 2

MIXED = dt2(BF16, F16)   # the mixed 16-bit mode: forward tensors f16, gradients bf16
NSHARD = 2
WGRAD_GROUP_MAX = 8
SRC_PLAIN, SRC_BN, SRC_BNBWD, SRC_BNADD = 0, 1, 2, 3
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class Src(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("mode", i32), ("relu", i32), ("stats", vp), ("rstats", vp),
                ("gamma", vp), ("beta", vp), ("rmean", vp), ("rvar", vp), ("inv_count", f32), ("eps", f32)]


class Conv(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("Hi", i32), ("Wi", i32), ("Ci", i32), ("Ho", i32), ("Wo", i32),
                ("Co", i32), ("ks", i32), ("stride", i32), ("stuff", i32), ("TH", i32), ("TW", i32), ("shape", i32),
                ("src", Src), ("w", vp), ("out", vp), ("bias", vp), ("out_relu", i32), ("out_stats", vp),
                ("addend", vp), ("mask_y", vp), ("mask_bn", Src), ("red", vp), ("mask_z", vp),
                ("src_out", vp), ("ydtype", i32), ("pad_", i32)]


class Wgrad(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("Hi", i32), ("Wi", i32), ("Ci", i32), ("Ho", i32), ("Wo", i32),
                ("Co", i32), ("ks", i32), ("stride", i32), ("TH", i32), ("TW", i32), ("nsplit", i32),
                ("h", Src), ("g", Src), ("partial", vp), ("ydtype", i32)]


class WgradGroup(C.Structure):
    _fields_ = [("n", i32), ("pad_", i32), ("p", C.POINTER(Wgrad) * 8)]


class Term(C.Structure):
    _fields_ = [("src", Src), ("shift", i32)]


class Fuse(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("nterms", i32), ("relu", i32),
                ("t", Term * 4), ("out", vp)]


class FuseBwd(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("ngrads", i32), ("relu", i32),
                ("nbn", i32), ("dz", vp * 4), ("z", vp), ("du", vp), ("bn", Src * 4), ("rstats", vp * 4), ("ydtype", i32), ("pad_", i32)]


class UpBwd(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("shift", i32),
                ("du", vp), ("dt", vp), ("bn", Src), ("rstats", vp), ("ydtype", i32), ("pad_", i32)]


class WPrep(C.Structure):
    _fields_ = [("src_off", i64), ("fwd_off", i64), ("bwd_off", i64), ("Co", i32), ("Ci", i32), ("ks", i32),
                ("Cip", i32), ("patch", i32), ("blk0", i32)]


class Slab(C.Structure):
    _fields_ = [("part_off", i64), ("grad_off", i64), ("nsplit", i32), ("Co", i32), ("Ci", i32), ("ks", i32),
                ("Cip", i32), ("patch", i32), ("blk0", i32), ("pad", i32)]


class BNRec(C.Structure):
    _fields_ = [("stats_off", i64), ("param_off", i64), ("buf_off", i64), ("C", i32), ("inv_count", f32)]


class Patch(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("stride", i32), ("pad_", i32), ("img", vp), ("out", vp),
                ("mean3", vp), ("std3", vp)]


class PatchBwd(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("stride", i32), ("pad_", i32), ("dpatch", vp), ("dimg", vp),
                ("std3", vp)]


class Head(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("Ci", i32), ("J", i32), ("x", vp), ("w", vp),
                ("bias", vp), ("out", vp)]


class HeadBwd(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("H", i32), ("W", i32), ("Ci", i32), ("J", i32), ("nblk", i32), ("pad_", i32),
                ("x", vp), ("w", vp), ("dout", vp), ("dx", vp), ("partial", vp)]


class DetImage(C.Structure):
    _fields_ = [("src", vp), ("kind", i32), ("old_h", i32), ("old_w", i32), ("new_h", i32), ("new_w", i32), ("pad_", i32),
                ("scale_y", C.c_double), ("scale_x", C.c_double)]


class DetPointwise(C.Structure):
    _fields_ = [("x", vp), ("w", vp), ("bias", vp), ("in_scale", vp), ("residual", vp), ("out", vp), ("M", i64),
                ("out_img_stride", i64), ("out_row_stride", i64), ("out_off", i64), ("HW", i32), ("Ci", i32), ("Co", i32),
                ("Kp", i32), ("Np", i32), ("act", i32)]


class DetPointwise16(C.Structure):
    _fields_ = [("x", vp), ("w", vp), ("bias", vp), ("in_scale", vp), ("residual", vp), ("out", vp), ("M", i64),
                ("out_img_stride", i64), ("out_row_stride", i64), ("out_off", i64), ("HW", i32), ("Ci", i32), ("Co", i32),
                ("Kp", i32), ("Np", i32), ("act", i32), ("dtype", i32), ("out_f32", i32)]


class DetPointwiseBwd(C.Structure):
    _fields_ = [("x", vp), ("w", vp), ("dy", vp), ("dx", vp), ("dw", vp), ("db", vp), ("partial", vp), ("M", i64),
                ("dy_img_stride", i64), ("dy_row_stride", i64), ("dy_off", i64), ("HW", i32), ("Ci", i32), ("Co", i32),
                ("Kp", i32), ("Np", i32), ("pad_", i32)]


class DetPointwise16Bwd(C.Structure):
    _fields_ = [("x", vp), ("wt", vp), ("dy", vp), ("dx", vp), ("dw", vp), ("db", vp), ("partial", vp), ("M", i64),
                ("dy_img_stride", i64), ("dy_row_stride", i64), ("dy_off", i64), ("HW", i32), ("Ci", i32), ("Co", i32),
                ("Kp", i32), ("Np", i32), ("xdtype", i32), ("dy_f32", i32), ("pad_", i32)]


class DetTerm(C.Structure):
    _fields_ = [("x", vp), ("mode", i32), ("H", i32), ("W", i32), ("pad_", i32)]


class DetFuse(C.Structure):
    _fields_ = [("B", i32), ("H", i32), ("W", i32), ("C", i32), ("nterms", i32), ("pad_", i32), ("t", DetTerm * 3), ("wparam", vp),
                ("out", vp)]


class Op(C.Structure):
    _fields_ = [("kind", i32), ("stream", i32), ("desc", vp), ("nwait", i32), ("wait", i32 * 8), ("record", i32)]


class ReduceRange(C.Structure):
    _fields_ = [("partials", vp), ("grads", vp), ("tab", vp), ("n", i32), ("blk_base", i32), ("nblocks", i32), ("pad_", i32)]


class BNRange(C.Structure):
    _fields_ = [("rstats", vp), ("grads", vp), ("tab", vp), ("n", i32), ("pad_", i32)]


OP_KIND = {"stl_conv_forward": 0, "stl_conv_wgrad": 1, "stl_fuse_forward": 2, "stl_fuse_backward": 3,
           "stl_upsample_backward": 4, "stl_patch3x3": 5, "stl_head_forward": 6, "stl_head_backward": 7,
           "stl_reduce_slabs_range": 8, "stl_bn_grads_range": 9, "stl_conv_wgrad_group": 10,   # 11, 12: retired, not reused
           "stl_patch3x3_backward": 13}

# name -> argtypes (restype is always int unless noted); every symbol include/stlpose_hip.h declares
SIGNATURES = {
    "stl_conv_forward": [C.POINTER(Conv), vp],
    "stl_conv_plan": [C.POINTER(Conv)],
    "stl_conv_bnadd_ok": [C.POINTER(Conv)],
    "stl_conv_wgrad": [C.POINTER(Wgrad), vp],
    "stl_wgrad_chunk": [C.POINTER(Wgrad)],
    "stl_conv_wgrad_group": [C.POINTER(WgradGroup), vp],
    "stl_fuse_forward": [C.POINTER(Fuse), vp],
    "stl_fuse_backward": [C.POINTER(FuseBwd), vp],
    "stl_upsample_backward": [C.POINTER(UpBwd), vp],
    "stl_patch3x3": [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp],
    "stl_patch3x3_backward": [i32, vp, vp, i32, i32, i32, i32, vp, vp],
    "stl_head_forward": [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "stl_head_backward": [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "stl_mse_loss": [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, f32, vp],
    "stl_gaussian_targets": [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, vp],
    "stl_heatmap_argmax": [vp, vp, vp, vp, i32, i32, i32, vp],
    "stl_flip_merge": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_flip_merge_backward": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_final_preds": [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_eval_tail": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, vp],
    "stl_eval_affine": [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp],
    "stl_weight_prep": [i32, vp, vp, vp, i32, i32, vp],
    "stl_reduce_slabs": [vp, vp, vp, i32, i32, vp],
    "stl_reduce_slabs_range": [C.POINTER(ReduceRange), vp],
    "stl_bn_running_update": [vp, vp, vp, vp, i32, f32, vp, vp],
    "stl_bn_param_grads": [vp, vp, vp, i32, vp],
    "stl_adam_step": [vp, vp, vp, vp, i64, vp, vp, vp, vp],
    "stl_sgd_step": [vp, vp, vp, i64, vp, vp, vp, vp],
    "stl_affine_crop": [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp],
    "stl_pose_augment": [vp, vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, C.c_double, C.c_double, i32, C.c_double, i32, i32,
                         vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "stl_maxpool2x2": [i32, vp, vp, i32, i32, i32, i32, vp],
    "stl_l1_partial": [i32, vp, vp, i64, vp, i32, vp],
    "stl_l2_partial": [i32, vp, vp, i64, vp, i32, vp],
    "stl_maxpool2x2_backward": [i32, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "stl_l2_backward": [i32, vp, vp, vp, i64, vp, i32, vp],
    "stl_bilinear_nchw": [vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "stl_sum_partials": [vp, i32, C.c_double, vp, i32, vp],
    "stl_nchw_to_nhwc": [i32, vp, vp, i32, i32, i32, i32, vp],
    "stl_nhwc_to_nchw": [i32, vp, vp, i32, i32, i32, i32, vp],
    "stl_program_create": [C.POINTER(Op), i32, i32, C.POINTER(vp)],
    "stl_program_run": [vp, C.POINTER(vp)],
    "stl_program_run_range": [vp, C.POINTER(vp), i32, i32],
    "stl_program_destroy": [vp],
    "stl_program_wait_op": [vp, i32, vp],
    "stl_selftest_mfma": [vp, vp],
    "stl_pose_vectors": [vp, i64, i32, vp, i32, i32, i32, vp],
    "stl_pose_distances": [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "stl_pose_topk_workspace": [i32, i32, i32, i32],
    "stl_pose_topk": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp],
    "stl_pose_rank": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp],
    "stl_pose_rank_any_workspace": [i32, i32],
    "stl_pose_rank_any": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, i64, vp],
    "stl_box_select": [vp, vp, vp, vp, i32, i64, i32, i64, i32, f32, C.c_double, vp, vp, vp],
    "stl_heatmap_resize_argmax": [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "stl_box_ap_match": [vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, i64, i32, i32, vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                         vp, vp, vp, vp, vp, vp, vp],
    "stl_box_ap_accumulate": [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, C.POINTER(i32), i32, C.POINTER(C.c_double), i32, vp, vp, vp],
    "stl_pose_rescore_nms": [vp, i32, i32, vp, vp, i32, i64, i32, C.c_double, C.c_double, C.POINTER(C.c_double), vp, vp, vp, vp],
    "stl_oks_ap_match": [vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, i64, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                         C.POINTER(C.c_double), vp, vp, vp, vp, vp, vp, vp],
    "stl_det_preprocess": [vp, i32, i32, vp, vp],
    "stl_det_stem": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_det_dwconv": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "stl_det_se": [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp],
    "stl_det_se_workspace": [i32],
    "stl_det_pointwise": [C.POINTER(DetPointwise), vp],
    "stl_det_fuse": [C.POINTER(DetFuse), vp],
    "stl_det_stem16": [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_det_dwconv16": [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "stl_det_dw16_parts": [i32],
    "stl_det_se16": [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp],
    "stl_det_pointwise16": [C.POINTER(DetPointwise16), vp],
    "stl_det_fuse16": [C.POINTER(DetFuse), i32, vp],
    "stl_det_decode": [vp, vp, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp],
    "stl_det_nms": [vp, vp, vp, i32, C.c_double, vp, vp, vp, vp],
    "stl_det_nms_workspace": [i32],
    "stl_det_pointwise_train": [C.POINTER(DetPointwise), vp, vp],
    "stl_det_loss": [vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp],
    "stl_det_pointwise_bwd_data": [C.POINTER(DetPointwiseBwd), vp],
    "stl_det_pointwise_bwd_weight": [C.POINTER(DetPointwiseBwd), vp],
    "stl_det_pointwise_bwd_slabs": [i64],
    "stl_det_dwconv_bwd_data": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_det_dwconv_bwd_weight": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_det_dwconv_bwd_parts": [i64],
    "stl_det_pointwise16_train": [C.POINTER(DetPointwise16), vp, vp],
    "stl_det_pointwise16_bwd_data": [C.POINTER(DetPointwise16Bwd), vp],
    "stl_det_pointwise16_bwd_weight": [C.POINTER(DetPointwise16Bwd), vp],
    "stl_det_pointwise16_bwd_slabs": [i64],
    "stl_det_dwconv16_bwd_data": [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "stl_det_dwconv16_bwd_weight": [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "stl_det_dwconv16_bwd_parts": [i64],
    "stl_adain_input": [i32, vp, vp, i32, i32, i32, vp],
    "stl_reflect_gather": [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp],
    "stl_adain_stats": [i32, vp, i32, i32, i32, i32, i32, i32, vp, f32, vp, vp, vp, vp],
    "stl_adain_affine": [vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp],
    "stl_adain_output": [i32, vp, vp, i32, i32, i32, i32, i32, vp],
    "stl_version": [],
}

# include/stlpose_hip_debug.h: exported by the stamped diagnostic build only (STLPOSE_HIP_LIB=.../libstlpose_hip_stamps.so)
DEBUG_SIGNATURES = {"stl_debug_conv_stamps": [vp], "stl_debug_conv_stamps2": [vp], "stl_debug_wgrad_stamps": [vp],
                    "stl_debug_wgrad_stamps2": [vp]}

INT64_FUNCS = ("stl_det_nms_workspace", "stl_pose_rank_any_workspace")   # int64_t f(...)
STRING_FUNCS = ("stl_last_error", "stl_build_id", "stl_last_kernel")   # const char* f(void)

_lib = None


def lib() -> C.CDLL:
    """Load the HIP library (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m stlpose_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
        l = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the ABI and this table disagree
            fn.argtypes = args
            fn.restype = C.c_int64 if name in INT64_FUNCS else C.c_int
        for name, args in DEBUG_SIGNATURES.items():
            if hasattr(l, name):
                getattr(l, name).argtypes, getattr(l, name).restype = args, C.c_int
        for name in STRING_FUNCS:
            fn = getattr(l, name)
            fn.argtypes = []
            fn.restype = C.c_char_p
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise RuntimeError(f"stlpose_hip {what}: {lib().stl_last_error().decode()}")


def call(name: str, *args) -> None:
    check(getattr(lib(), name)(*args), name)
