/*
 * stlpose_hip_math.h -- the values of stl_conv.math (stlpose_hip.h): how a conv launch multiplies its operands.  Written in the C
 * subset of stlpose_hip.h and read by the same reader (stlpose_amd/capi.py: capi.MATH_NATIVE, capi.MATH_BF16X3).
 *
 * STL_MATH_BF16X3: fp32 tensors (dtype STL_F32: stored, staged, transformed on load and accumulated as fp32, the fp32 weight
 * layouts) multiplied on the bf16 matrix cores.  Each operand is split into hi = bf16(x) and lo = bf16(x - hi), both rounded to
 * nearest even, and the product is taken as lo*hi + hi*lo + hi*hi on one fp32 accumulator, smallest term first: three
 * v_mfma_f32_16x16x16_bf16 per 64-byte K slice instead of four v_mfma_f32_16x16x4_f32.  The lo*lo term and the residue of the
 * split are about 2^-16 per product: inside the inference tolerance (heat maps within 1e-3, argmax equal), outside the training
 * one.  So: stl_conv_forward / stl_conv_plan take it with dtype STL_F32 in forward launches only; with any other
 * dtype, with a BNBWD source or with stuff = 1 it is an error that names the field.
 * hi is rounded from x clamped to bf16's finite range, so an Inf operand multiplies as an Inf (lo = Inf) and |x| above bf16's
 * largest finite value splits exactly; a NaN stays a NaN; zeros stay zeros.
 */
#ifndef STLPOSE_HIP_MATH_H
#define STLPOSE_HIP_MATH_H

#define STL_MATH_NATIVE 0
#define STL_MATH_BF16X3 1

#endif
