// Shared by the one-lane-per-item kernels of the mesh and cloud tools (csrc/meshtopo.hip, csrc/meshsimp.hip, csrc/orient.hip,
// csrc/register.hip, csrc/segment.hip): the wave-aggregated counter, the fixed-order fp64 wavefront sum and the order-preserving
// integer form of a float.  (Not in common.h: build.kernel_hash covers that file for the roofline kernels, whose committed counter
// records a change there would void.)
#pragma once
#include "common.h"

// the lanes' 0 / 1 flags become one integer atomic per wavefront; every lane of the wavefront must call it
template <typename T>
__device__ __forceinline__ void wave_count(bool flag, T* total) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & (NKSR_WAVE - 1)) == (unsigned)(__ffsll((long long)m) - 1))
        __hip_atomic_fetch_add(total, (T)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the fp64 sum over the 64 lanes by a butterfly: both partners add the same two numbers, so all lanes end with the same bits, in an
// order that depends on nothing but the lanes (csrc/register.hip, csrc/segment.hip); every lane of the wavefront must call it
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = NKSR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// fp32 -> uint32 keeping the order (negative: all bits flipped, otherwise the sign bit set; -0 counted as +0), and back.  A compare and
// a select, no arithmetic: a NaN keeps its payload and nothing depends on the floating-point mode.
__host__ __device__ __forceinline__ uint32_t ordered_bits(float x) {
    float y = x == 0.0f ? 0.0f : x;
    uint32_t b;
    memcpy(&b, &y, sizeof b);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ __forceinline__ float ordered_float(uint32_t u) {
    const uint32_t b = u & 0x80000000u ? u & 0x7FFFFFFFu : ~u;
    float x;
    memcpy(&x, &b, sizeof x);
    return x;
}
