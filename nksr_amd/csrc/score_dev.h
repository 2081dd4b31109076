// The RANSAC scorer of csrc/segment.hip (planes against points) and csrc/global_register.hip (poses against pairs): every hypothesis
// against every item in one launch, integer counts.
//
//   k_hypothesis_score<Model>  a workgroup holds Model::CHUNK hypotheses in LDS (Model::WIDTH doubles each), a lane holds Model::ITEMS
//                              items in registers and loops over the hypotheses; ballot + popcount per wavefront into integer LDS
//                              counters, one integer atomicAdd per (workgroup, hypothesis) at the end.  Integer sums do not depend
//                              on the order.  A degenerate hypothesis counts -1.
// A Model gives:  WIDTH, ITEMS, CHUNK, MAX_H (the hypotheses one launch takes);  Items (the arrays the items are read from) with
// missing() (a NULL among them), Item;  load(items, i, on, item): item i, or -- on false, a lane past the end -- one whose NaNs fail every comparison;
// inlier(hyp, item, t);  degenerate(hyp);  N_NAME / H_NAME: what the two sizes are called in the error messages.
#pragma once
#include "common.h"

#define SCORE_BLOCK 256

template <class Model>
__global__ void __launch_bounds__(SCORE_BLOCK) k_hypothesis_score(typename Model::Items items, int64_t n, const double* __restrict__ hyps,
                                                                  int n_hyp, double t, int32_t* counts) {
    constexpr int WAVES = SCORE_BLOCK / NKSR_WAVE, WIDTH = Model::WIDTH, ITEMS = Model::ITEMS, CHUNK = Model::CHUNK;
    __shared__ double s_hyp[CHUNK * WIDTH];
    __shared__ int32_t s_count[WAVES][CHUNK];
    const int h0 = blockIdx.y * CHUNK;
    const int nh = n_hyp - h0 < CHUNK ? n_hyp - h0 : CHUNK;
    for (int k = threadIdx.x; k < nh * WIDTH; k += SCORE_BLOCK) s_hyp[k] = hyps[(int64_t)h0 * WIDTH + k];
    typename Model::Item item[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t i = ((int64_t)blockIdx.x * ITEMS + k) * SCORE_BLOCK + threadIdx.x;
        Model::load(items, i, i < n, item[k]);
    }
    __syncthreads();
    const int wave = threadIdx.x / NKSR_WAVE, lane = threadIdx.x % NKSR_WAVE;
    for (int h = 0; h < nh; ++h) {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) cnt += __popcll(__ballot(Model::inlier(s_hyp + WIDTH * h, item[k], t)));
        if (lane == 0) s_count[wave][h] = cnt;
    }
    __syncthreads();
    for (int h = threadIdx.x; h < nh; h += SCORE_BLOCK) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) total += s_count[w][h];
        if (Model::degenerate(s_hyp + WIDTH * h)) total = blockIdx.x == 0 ? -1 : 0;          // (the counts start at 0: -1 in the end)
        if (total) atomicAdd(counts + h0 + h, total);
    }
}

// the checks every entry point with n items and a distance threshold begins with
static int threshold_args(const char* who, const char* n_name, int64_t n, double threshold) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: %s=%lld outside [0, 2^31)", who, n_name, (long long)n);
    if (!(threshold >= 0.0) || !(threshold < (double)INFINITY))
        return nksr_set_error(NKSR_ERR_ARG, "%s: the distance threshold must be finite and not negative", who);
    return NKSR_OK;
}

// checks, zeroed counts, launch.  `t`: the threshold as the kernel compares it (the checks are made on `threshold`)
template <class Model>
static int hypothesis_score(const char* who, typename Model::Items items, int64_t n, const double* hyps, int64_t n_hyp, double threshold,
                            double t, int32_t* counts_out, void* stream) {
    if (int rc = threshold_args(who, Model::N_NAME, n, threshold)) return rc;
    if (n_hyp < 0 || n_hyp > Model::MAX_H)
        return nksr_set_error(NKSR_ERR_ARG, "%s: %s=%lld outside [0, %d]", who, Model::H_NAME, (long long)n_hyp, Model::MAX_H);
    if (n_hyp == 0) return NKSR_OK;
    if (!hyps || !counts_out || (n > 0 && items.missing())) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL arrays", who);
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(counts_out, 0, sizeof(int32_t) * (size_t)n_hyp, st));
    // (n = 0: one column of workgroups still marks the degenerate hypotheses)
    const dim3 grid(n > 0 ? nksr_blocks(n, SCORE_BLOCK * Model::ITEMS) : 1, nksr_blocks(n_hyp, Model::CHUNK));
    hipLaunchKernelGGL(k_hypothesis_score<Model>, grid, dim3(SCORE_BLOCK), 0, st, items, n, hyps, (int)n_hyp, t, counts_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
