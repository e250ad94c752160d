"""ctypes binding of libstlpose_hip.so, read from include/stlpose_hip.h at import (``cheader.Header``).

The header is the only statement of the C ABI.  From it come the constants (``STL_NSHARD`` is ``capi.NSHARD``), one
``ctypes.Structure`` per ``typedef struct`` (``stl_conv`` is ``capi.Conv``, see ``CLASS_NAMES``) and ``SIGNATURES`` / ``RESTYPES`` of
every prototype.  Written here are only what the header cannot say: the Python names, which structs are device-table records, and
the string-keyed maps.

The product path has no CPU fallback: if the HIP library is missing this module raises at
import-of-symbols time (``lib()``), loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from .cheader import Header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STLPOSE_HIP_LIB") or os.path.join(_HERE, "libstlpose_hip.so")   # override: A/B of two builds
INCLUDE = os.path.join(_HERE, "..", "include")
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# C struct -> Python class
CLASS_NAMES = {
    "stl_src": "Src", "stl_conv": "Conv", "stl_wgrad": "Wgrad", "stl_wgrad_io": "WgradIO", "stl_wgrad_group": "WgradGroup",
    "stl_term": "Term", "stl_fuse": "Fuse", "stl_fuse_bwd": "FuseBwd", "stl_upbwd": "UpBwd", "stl_wprep": "WPrep", "stl_slab": "Slab",
    "stl_bnrec": "BNRec", "stl_reduce_range": "ReduceRange", "stl_bn_range": "BNRange", "stl_patch": "Patch",
    "stl_patch_bwd": "PatchBwd", "stl_head": "Head", "stl_head_bwd": "HeadBwd", "stl_op": "Op", "StlDetImage": "DetImage",
    "StlDetPointwise": "DetPointwise", "StlDetTerm": "DetTerm", "StlDetFuse": "DetFuse", "StlDetPointwise16": "DetPointwise16",
    "StlDetPointwiseBwd": "DetPointwiseBwd", "StlDetPointwise16Bwd": "DetPointwise16Bwd"}
# The records of device tables: the host fills arrays of them, copies those to the device and passes the device address, so a
# pointer to one is a c_void_p.  A pointer to any other struct is a host descriptor, POINTER(Class), passed with byref.  This is
# the one classification the header does not carry.
DEVICE_RECORDS = ("stl_wprep", "stl_slab", "stl_bnrec", "StlDetImage")

HEADER = Header(os.path.join(INCLUDE, "stlpose_hip.h"), CLASS_NAMES, DEVICE_RECORDS)
if set(HEADER.structs) != set(CLASS_NAMES):
    raise ImportError(f"capi.CLASS_NAMES and the structs of include/stlpose_hip.h differ: {sorted(set(HEADER.structs) ^ set(CLASS_NAMES))}")
globals().update({name[len("STL_"):]: value for name, value in HEADER.constants.items()})   # F32, NSHARD, SRC_BNADD, OP_CONV, ...
globals().update({cls.__name__: cls for cls in HEADER.structs.values()})                    # Src, Conv, Wgrad, ...
SIGNATURES, RESTYPES = HEADER.signatures, HEADER.restypes   # name -> argtypes, name -> restype; every symbol of the header
INT64_FUNCS = tuple(n for n, r in RESTYPES.items() if r is C.c_int64)     # int64_t f(...)
STRING_FUNCS = tuple(n for n, r in RESTYPES.items() if r is C.c_char_p)   # const char* f(void)
# include/stlpose_hip_debug.h: exported by the stamped diagnostic build only (STLPOSE_HIP_LIB=.../libstlpose_hip_stamps.so)
DEBUG_SIGNATURES = Header(os.path.join(INCLUDE, "stlpose_hip_debug.h")).signatures
# include/stlpose_hip_detections.h: the detector's device tail (csrc/detections.hip), part of the product library
DETECTIONS = Header(os.path.join(INCLUDE, "stlpose_hip_detections.h"))
# include/stlpose_hip_det_batch.h: detector batches built on the device (csrc/det_batch.hip), part of the product library
DET_BATCH = Header(os.path.join(INCLUDE, "stlpose_hip_det_batch.h"))
globals().update({name[len("STL_"):]: value for name, value in DET_BATCH.constants.items()})   # DET_BATCH_MAX, DET_BATCH_SIDE
# include/stlpose_hip_det_bifpn.h: the BiFPN node's backward (csrc/detector_bifpn.hip), part of the product library; it takes
# StlDetFuse from stlpose_hip.h
DET_BIFPN = Header(os.path.join(INCLUDE, "stlpose_hip_det_bifpn.h"), {"StlDetFuseBwd": "DetFuseBwd"}, base=HEADER)
DetFuseBwd = DET_BIFPN.structs["StlDetFuseBwd"]
# include/stlpose_hip_det_mbconv.h: the new pieces of an MBConv block's backward (csrc/detector_mbconv.hip), part of the product library
DET_MBCONV = Header(os.path.join(INCLUDE, "stlpose_hip_det_mbconv.h"))
# include/stlpose_hip_math.h: the values of stl_conv.math
MATH = Header(os.path.join(INCLUDE, "stlpose_hip_math.h"))
globals().update({name[len("STL_"):]: value for name, value in MATH.constants.items()})   # MATH_NATIVE, MATH_BF16X3

DTYPES = {F32: (4, torch.float32), BF16: (2, torch.bfloat16), F16: (2, torch.float16)}   # code -> (bytes per element, torch dtype)


def dt2(grad_dtype: int, fwd_dtype: int) -> int:
    """STL_DT2: two element types in one int (low byte: gradient-side tensors, bits 8-15: forward-side tensors if different)."""
    return grad_dtype | ((fwd_dtype if fwd_dtype != grad_dtype else 0) << 8)


MIXED = dt2(BF16, F16)   # the mixed 16-bit mode: forward tensors f16, gradients bf16
# A compute mode of the Python layer may carry an stl_conv.math value above the two element types (bits 16-23): "fp32x3" is fp32
# tensors whose conv launches multiply split bf16 operands on the 16-bit matrix cores.  Inference only (X3_NO_GRADIENTS).
F32X3 = F32 | (MATH_BF16X3 << 16)
X3_NO_GRADIENTS = ("compute_dtype='fp32x3' is inference only: gradients need the third bf16 piece of each operand (the two-piece "
                   "split is 16-30x fp32's gradient error); train and differentiate with compute_dtype=\"fp32\".")


def math_of(code: int) -> int:
    """The STL_MATH_* value of a compute-mode code (0 for every mode but F32X3)."""
    return (code >> 16) & 0xff

# pose retrieval
POSE_APPROACH = {"all_kpts": POSE_ALL_KPTS, "full_body": POSE_FULL_BODY, "upper_body": POSE_UPPER_BODY}
POSE_DIM = {"all_kpts": 34, "full_body": 26, "upper_body": 18}
POSE_METHOD = {"euclidean": POSE_EUCLIDEAN, "cosine": POSE_COSINE, "manhattan": POSE_MANHATTAN, "confidence": POSE_CONFIDENCE,
               "oks": POSE_OKS, "l2sq": POSE_L2SQ, "cos_normalised": POSE_COS_NORMALISED}
POSE_PEN = {"zero_coord": POSE_PEN_ZERO_COORD, "none": POSE_PEN_NONE, "mean": POSE_PEN_MEAN, "max": POSE_PEN_MAX}
POSE_SUM_ORDER = {"numpy": POSE_SUM_NUMPY, "reference": POSE_SUM_SERIAL}
# the entry point an op of a native program stands for -> its STL_OP_* kind
OP_KIND = {"stl_conv_forward": OP_CONV, "stl_conv_wgrad": OP_WGRAD, "stl_fuse_forward": OP_FUSE, "stl_fuse_backward": OP_FUSE_BWD,
           "stl_upsample_backward": OP_UP_BWD, "stl_patch3x3": OP_PATCH, "stl_head_forward": OP_HEAD, "stl_head_backward": OP_HEAD_BWD,
           "stl_reduce_slabs_range": OP_REDUCE_RANGE, "stl_bn_grads_range": OP_BN_GRADS_RANGE,
           "stl_conv_wgrad_group": OP_WGRAD_GROUP, "stl_patch3x3_backward": OP_PATCH_BWD}

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
            fn = getattr(l, name)  # AttributeError if the library lacks a symbol of the header
            fn.argtypes, fn.restype = args, RESTYPES[name]
        for header in (DETECTIONS, DET_BATCH, DET_BIFPN, DET_MBCONV):
            for name, args in header.signatures.items():
                fn = getattr(l, name)
                fn.argtypes, fn.restype = args, header.restypes[name]
        for name, args in DEBUG_SIGNATURES.items():
            if hasattr(l, name):
                getattr(l, name).argtypes, getattr(l, name).restype = args, C.c_int
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise RuntimeError(f"stlpose_hip {what}: {lib().stl_last_error().decode()}")


def call(name: str, *args) -> None:
    check(getattr(lib(), name)(*args), name)
