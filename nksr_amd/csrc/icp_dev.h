// The terms of one ICP correspondence, shared by the kernels that write rows of NKSR_ICP_FIELDS sums (csrc/register.hip: pairs found
// by a search; csrc/global_register.hip: pairs that are given): the transform and the terms are stated ONCE, formed without fused
// multiply-adds in the order include/nksr_hip.h gives.
//
// block_row_sums is the end of every kernel that writes such a row (k_icp_accumulate, k_corr_accumulate, and k_plane_moments of
// csrc/segment.hip): THE statement of the order in which a workgroup adds its lanes' terms.
#pragma once
#include "common.h"
#include "wave_dev.h"

static_assert(NKSR_ICP_BLOCK % NKSR_WAVE == 0 && NKSR_ICP_FIELDS <= NKSR_ICP_BLOCK, "whole wavefronts, one lane per field at the end");

// term[0 .. NF) of the NKSR_ICP_BLOCK lanes of the workgroup -> row blockIdx.x of partials, NKSR_ICP_FIELDS wide, zero above NF.  Per
// field: the 64 lanes of a wavefront by the butterfly of wave_sum_f64 (xor 32, 16, ... 1), then the wavefronts in wave order starting
// from 0.0.  Every lane of the workgroup must call it (a lane without an item carries zeros).  STRIDE: the width of the LDS rows.
template <int NF, int STRIDE = NF>
__device__ __forceinline__ void block_row_sums(const double* term, double* __restrict__ partials) {
    static_assert(NF <= STRIDE && STRIDE <= NKSR_ICP_FIELDS, "the fields of one row");
    constexpr int WAVES = NKSR_ICP_BLOCK / NKSR_WAVE;
    __shared__ double s_red[WAVES][STRIDE];
    const int wave = threadIdx.x / NKSR_WAVE, lane = threadIdx.x % NKSR_WAVE;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const double v = wave_sum_f64(term[f]);
        if (lane == 0) s_red[wave][f] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < NKSR_ICP_FIELDS) {
        double v = 0.0;
        if ((int)threadIdx.x < NF)
            for (int w = 0; w < WAVES; ++w) v += s_red[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * NKSR_ICP_FIELDS + threadIdx.x] = v;
    }
}

// p = R s + t, every product and sum rounded on its own
__device__ __forceinline__ void icp_transform(const double* __restrict__ T, const float s[3], double p[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = T[4 * a] * (double)s[0] + T[4 * a + 1] * (double)s[1];
        const double v = u + T[4 * a + 2] * (double)s[2];
        p[a] = v + T[4 * a + 3];
    }
}

// the terms of one correspondence (p, q) -- and of its normal n for the plane method -- about the centre c
template <int METHOD>
__device__ __forceinline__ void icp_terms(const double p[3], const double q[3], const float* __restrict__ nrm, const double c[3],
                                          double term[NKSR_ICP_FIELDS]) {
#pragma clang fp contract(off)
    const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    const double pp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    term[NKSR_ICP_COUNT] = 1.0;
    const double dxy = d[0] * d[0] + d[1] * d[1];
    term[NKSR_ICP_D2] = dxy + d[2] * d[2];
    if (METHOD == 0) {
        const double qq[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            term[NKSR_ICP_PT_P + a] = pp[a];
            term[NKSR_ICP_PT_Q + a] = qq[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) term[NKSR_ICP_PT_PQ + 3 * a + b] = pp[a] * qq[b];
        }
    } else {
        const double n[3] = {(double)nrm[0], (double)nrm[1], (double)nrm[2]};
        const double rxy = n[0] * d[0] + n[1] * d[1];
        const double r = rxy + n[2] * d[2];
        const double J[6] = {pp[1] * n[2] - pp[2] * n[1], pp[2] * n[0] - pp[0] * n[2], pp[0] * n[1] - pp[1] * n[0], n[0], n[1], n[2]};
        int k = NKSR_ICP_PL_JJ;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) term[k++] = J[a] * J[b];
            term[NKSR_ICP_PL_JR + a] = J[a] * r;
        }
        term[NKSR_ICP_PL_RR] = r * r;
    }
}
