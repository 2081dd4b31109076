// Shared by the conjugate-gradient loop (csrc/pcg.hip) and the coarse-level block preconditioner (csrc/cheb.hip): the per-segment
// scalars the Chebyshev kernels look at, and the fixed-order fp64 reductions.  (Not in common.h: build.kernel_hash covers that file
// for the roofline kernels, whose committed counter records a change there would void.)
#pragma once
#include "common.h"

#define PCG_BLOCK 256

// Independent diagonal blocks ("segments": the chunks of a batched chunk solve, nksr_segments_t) run their OWN conjugate gradients
// inside shared launches: scalars per segment, dot products reduced per segment in a fixed, SEGMENT-RELATIVE order (blocks of
// SPCG_BS unknowns counted from the start of each of the segment's index ranges, partial sums added in block order), so the
// iterates of a segment do not depend on which other segments share the launch; a converged segment freezes (its blocks return
// early) while the others go on.  One segment [0, M) is the ordinary solve.
struct SegScalars {
    double rz[2];
    double bb;
    double rel;
    int iter;
    int done;               // 1: converged (or empty right-hand side), 2: hard failure (r.z <= 0 with the Jacobi preconditioner too, NaN)
    int jacobi;             // 1: the coarse-level block lost definiteness for this segment (r.z <= 0): it went on with Jacobi alone
    int pad;
};

// the coarse-level block leaves this segment's slice of z alone: it has finished, or it went on with Jacobi (sc == NULL: no segment has)
__device__ __forceinline__ bool seg_skipped(const SegScalars* __restrict__ sc, int seg) { return sc && (sc[seg].done || sc[seg].jacobi); }

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// block-wide fp64 sum; result valid in thread 0.  sm must hold blockDim/64 doubles.
__device__ __forceinline__ double block_sum(double v, double* sm) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sm[w];
    return t;
}

// every block re-reduces the partial array in the same fixed order -> identical value everywhere
__device__ __forceinline__ double reduce_partials(const double* __restrict__ part, int nb, int stride, double* sm) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) v += part[(int64_t)i * stride];
    double t = block_sum(v, sm);
    __shared__ double bc;
    if (threadIdx.x == 0) bc = t;
    __syncthreads();
    return bc;
}
