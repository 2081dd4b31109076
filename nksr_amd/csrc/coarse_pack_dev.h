// The packed coarse block's drop rule and entry word, stated once for both of its producers -- the converter of the fp32 CSR
// (csrc/cheb.hip: k_cc_count / k_cc_pack) and the fill that emits it directly (csrc/assemble.hip: k_row_fill<NQ, true>) -- and for
// the kernels that read it (csrc/cheb.hip: k_cheb16_step, k_gersh_rows).  tests/test_gpu_coarse_direct.py compares the two
// producers word for word.  (Not in common.h: build.kernel_hash covers that file for the roofline kernels, whose committed counter
// records a change there would void.)
#pragma once
#include "common.h"
#include <hip/hip_fp16.h>

// Entries with |S_ij| < drop are left out (drop = 0 keeps all): the far corners of the 5 x 5 x 5 stencil carry 1e-2 .. 1e-6 of
// the diagonal and most of the bytes; the dropped matrix is still symmetric (S_ij and S_ji are the same bits) and the polynomial of
// it is still a fixed symmetric positive operator.
__device__ __forceinline__ __half cc_scaled(float v, float di, float dj) { return __float2half_rn(v * (di * dj)); }
__device__ __forceinline__ bool cc_keep(__half hv, float drop) { return fabsf(__half2float(hv)) >= drop; }

// one entry = half-precision value << 16 | column local to the row's segment (< 2^16)
__device__ __forceinline__ uint32_t cc_word(__half hv, uint32_t local_col) { return ((uint32_t)__half_as_ushort(hv) << 16) | local_col; }
__device__ __forceinline__ float cc_word_value(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w >> 16))); }
__device__ __forceinline__ int cc_word_col(uint32_t w) { return (int)(w & 0xFFFFu); }
