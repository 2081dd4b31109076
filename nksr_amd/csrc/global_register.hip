// Global registration from matched features (nksr_amd/global_register.py: cloud.match_features,
// cloud.registration_ransac_based_on_feature_matching).  include/nksr_hip.h states what every entry point computes.
//
//   k_feature_match    nksr_feature_match: the nearest row of B for every row of A in the 33-dimensional feature space, by brute force
//                      and by the DIRECT difference: D = sum_j (a_j - b_j)^2 in fp32, ascending j, no fused multiply-add.  (The
//                      expansion |a|^2 + |b|^2 - 2 a.b and the matrix cores that would serve it are left alone on purpose: the
//                      features are non-negative histograms that often nearly coincide, and the cancellation makes the argmin depend
//                      on the summation order.)  A lane keeps ONE row of A in 33 registers; the workgroup stages FM_TILE rows of B in
//                      LDS, two rows interleaved entry by entry and padded to 36 float2, so that a PAIR of rows is seventeen 16-byte
//                      reads, and all lanes read the SAME pair: a broadcast, no bank conflicts.  Per pair of rows a lane issues 17
//                      LDS reads against 99 packed fp32 operations -- the loop is bound by the arithmetic, so a second A row per
//                      lane would buy nothing and cost 33 more registers.  The lane sees its rows of B in ascending order and
//                      takes a new best on `<` alone: the lowest index among equal distances.
//                      The grid splits A over x and -- 196 workgroups would not fill 256 compute units at 50 000 rows -- B over y; the
//                      partial answers of a row meet in ONE 64-bit integer atomicMin on (bits of D) << 32 | b.  D is a sum of squares,
//                      never negative, so its bit pattern orders as an unsigned integer and the minimum is the smallest D, then the
//                      smallest b: independent of the order the workgroups run in.  k_feature_match_finish unpacks the keys.
//   PoseModel          nksr_pose_score: all hypotheses in one launch of k_hypothesis_score (score_dev.h), the scorer csrc/segment.hip
//                      runs on planes: integer counts, -1 for a transform that is not finite.
//   k_corr_accumulate  nksr_corr_accumulate: the inlier mask of ONE transform and the point-method rows of the ICP sums over its
//                      inliers (icp_dev.h: the same transform, the same terms, the same block_row_sums).
#include "common.h"
#include "icp_dev.h"
#include "score_dev.h"

// ---- A. feature matching -------------------------------------------------------------------------------------------------------------
#define FM_BLOCK 256
#define FM_TILE 128                 // rows of B in LDS, as 64 row PAIRS of 36 float2: 18 432 B
#define FM_PAIR 72                  // floats per staged pair of rows: 33 x (row 2p, row 2p + 1), padded to 36 float2 (16-byte reads)
#define FM_TARGET_BLOCKS 1024       // the grid is grown to about this many workgroups by splitting B (256 compute units x 4)
#define FM_NONE 0xFFFFFFFFFFFFFFFFull
static_assert(NKSR_FPFH_BINS == 33 && FM_PAIR == 72 && FM_TILE % 2 == 0, "sixteen float4 and one float2 per pair of rows");
typedef float fm_f4 __attribute__((ext_vector_type(4)));
typedef float fm_f2 __attribute__((ext_vector_type(2)));

// Two rows of B per trip: entry j of rows 2p and 2p + 1 lie side by side in LDS, so the differences, products and sums of the two rows
// are the two halves of packed fp32 instructions (v_pk_add_f32 / v_pk_mul_f32: the same IEEE operations, twice per issue; the loop is
// bound by the VALU).  Row 2p is compared first, `<` alone: ascending order as before.  An odd last row gets a partner of NaNs.
__global__ void __launch_bounds__(FM_BLOCK) k_feature_match(const float* __restrict__ A, int na, const float* __restrict__ B, int nb,
                                                            int rows_per_split, unsigned long long* keys) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float s_b[(FM_TILE / 2) * FM_PAIR];
    const int64_t i = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    float a[NKSR_FPFH_BINS];
#pragma unroll
    for (int j = 0; j < NKSR_FPFH_BINS; ++j) a[j] = i < na ? A[i * NKSR_FPFH_BINS + j] : NAN;         // (a lane past the end never matches)
    const int64_t lo64 = (int64_t)blockIdx.y * rows_per_split;
    const int lo = (int)lo64, hi = lo64 + rows_per_split < nb ? (int)(lo64 + rows_per_split) : nb;
    float best = INFINITY;
    int bi = -1;
    for (int t0 = lo; t0 < hi; t0 += FM_TILE) {
        const int rows = hi - t0 < FM_TILE ? hi - t0 : FM_TILE, pairs = (rows + 1) / 2;
        __syncthreads();                                // (the reads of the tile before are done)
        for (int e = threadIdx.x; e < 2 * pairs * NKSR_FPFH_BINS; e += FM_BLOCK) {
            const int r = e / NKSR_FPFH_BINS, j = e % NKSR_FPFH_BINS;
            s_b[(r >> 1) * FM_PAIR + 2 * j + (r & 1)] = r < rows ? B[(int64_t)t0 * NKSR_FPFH_BINS + e] : NAN;
        }
        __syncthreads();
        for (int p = 0; p < pairs; ++p) {
            const fm_f4* row = reinterpret_cast<const fm_f4*>(s_b + p * FM_PAIR);
            fm_f2 D = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const fm_f4 v = row[q];
                const fm_f2 a0 = {a[2 * q], a[2 * q]}, a1 = {a[2 * q + 1], a[2 * q + 1]};
                const fm_f2 d0 = a0 - v.xy, d1 = a1 - v.zw;
                D = D + d0 * d0;
                D = D + d1 * d1;
            }
            const fm_f2 al = {a[32], a[32]};
            const fm_f2 dl = al - *reinterpret_cast<const fm_f2*>(s_b + p * FM_PAIR + 64);
            D = D + dl * dl;
            if (D.x < best) { best = D.x; bi = t0 + 2 * p; }            // (false for a NaN and for +inf: such a row of A finds nothing)
            if (D.y < best) { best = D.y; bi = t0 + 2 * p + 1; }
        }
    }
    if (bi >= 0) atomicMin(keys + i, ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(uint32_t)bi);
}

__global__ void __launch_bounds__(FM_BLOCK) k_feature_match_finish(const unsigned long long* __restrict__ keys, int na, int32_t* __restrict__ idx,
                                                                   float* __restrict__ dist2) {
    const int64_t i = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    if (i >= na) return;
    const unsigned long long key = keys[i];
    idx[i] = key == FM_NONE ? -1 : (int32_t)(key & 0xFFFFFFFFull);
    dist2[i] = key == FM_NONE ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
}

extern "C" int nksr_feature_match(const float* A, int64_t na, const float* B, int64_t nb, uint64_t* keys_work, int32_t* idx_out,
                                  float* dist2_out, void* stream) {
    if (na < 0 || nb < 0 || na >= (1ll << 31) || nb >= (1ll << 31))
        return nksr_set_error(NKSR_ERR_ARG, "feature match: sizes outside [0, 2^31) (na=%lld, nb=%lld)", (long long)na, (long long)nb);
    if (na == 0) return NKSR_OK;
    if (!A || !keys_work || !idx_out || !dist2_out || (nb > 0 && !B)) return nksr_set_error(NKSR_ERR_ARG, "feature match: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(keys_work, 0xFF, sizeof(uint64_t) * (size_t)na, st));
    const int bx = nksr_blocks(na, FM_BLOCK);
    if (nb > 0) {
        const int tiles = nksr_blocks(nb, FM_TILE);
        int splits = (FM_TARGET_BLOCKS + bx - 1) / bx;
        splits = splits < 1 ? 1 : (splits > tiles ? tiles : splits);
        const int rows_per_split = ((tiles + splits - 1) / splits) * FM_TILE;          // whole tiles
        splits = nksr_blocks(nb, rows_per_split);
        hipLaunchKernelGGL(k_feature_match, dim3(bx, splits), dim3(FM_BLOCK), 0, st, A, (int)na, B, (int)nb, rows_per_split,
                           reinterpret_cast<unsigned long long*>(keys_work));
        NKSR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_feature_match_finish, dim3(bx), dim3(FM_BLOCK), 0, st, reinterpret_cast<const unsigned long long*>(keys_work),
                       (int)na, idx_out, dist2_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// ---- B. pose hypotheses ----------------------------------------------------------------------------------------------------------------
// e = (R p + t) - q, |e|^2 <= t2; moved [3] = R p + t
__device__ __forceinline__ bool pose_inlier(const double* __restrict__ T, const float p[3], const double q[3], double t2, double moved[3]) {
#pragma clang fp contract(off)
    icp_transform(T, p, moved);
    const double e[3] = {moved[0] - q[0], moved[1] - q[1], moved[2] - q[2]};
    const double xy = e[0] * e[0] + e[1] * e[1];
    return xy + e[2] * e[2] <= t2;
}
__device__ __forceinline__ bool pose_not_finite(const double* __restrict__ T) {
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 12; ++a) finite = finite && fabs(T[a]) < INFINITY;            // (false for a NaN)
    return !finite;
}

// the model of k_hypothesis_score (score_dev.h): 2 pairs a lane (6 floats + 6 doubles), 64 transforms a workgroup (6 KB, and 1 KB of
// counts); the threshold arrives squared
struct PoseModel {
    static constexpr int WIDTH = 12, ITEMS = 2, CHUNK = 64, MAX_H = NKSR_POSE_MAX_H;
    static constexpr const char* N_NAME = "n_pairs";
    static constexpr const char* H_NAME = "n_hyp";
    struct Items {
        const float* __restrict__ src;
        const float* __restrict__ tgt;
        bool missing() const { return !src || !tgt; }
    };
    struct Item { float p[3]; double q[3]; };
    static __device__ __forceinline__ void load(const Items& in, int64_t i, bool on, Item& it) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            it.p[a] = on ? in.src[i * 3 + a] : 0.f;
            it.q[a] = on ? (double)in.tgt[i * 3 + a] : (double)NAN;         // a lane past the end carries a NaN: no comparison with it holds
        }
    }
    static __device__ __forceinline__ bool inlier(const double* T, const Item& it, double t2) {
        double moved[3];
        return pose_inlier(T, it.p, it.q, t2, moved);
    }
    static __device__ __forceinline__ bool degenerate(const double* T) { return pose_not_finite(T); }
};

#define CA_FIELDS (NKSR_ICP_PT_PQ + 9)          // the fields the point method fills

__global__ void __launch_bounds__(NKSR_ICP_BLOCK) k_corr_accumulate(const float* __restrict__ src, const float* __restrict__ tgt, int64_t n,
                                                                    const double* __restrict__ T, const double* __restrict__ centre, double t2,
                                                                    uint8_t* __restrict__ mask, double* __restrict__ partials) {
    const int64_t i = (int64_t)blockIdx.x * NKSR_ICP_BLOCK + threadIdx.x;
    double term[NKSR_ICP_FIELDS];
#pragma unroll
    for (int f = 0; f < NKSR_ICP_FIELDS; ++f) term[f] = 0.0;
    if (i < n) {
        const float s[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
        const double q[3] = {(double)tgt[i * 3], (double)tgt[i * 3 + 1], (double)tgt[i * 3 + 2]};
        double p[3];
        const bool in = pose_inlier(T, s, q, t2, p);
        mask[i] = in ? 1 : 0;
        if (in) {
            const double c3[3] = {centre[0], centre[1], centre[2]};
            icp_terms<0>(p, q, nullptr, c3, term);
        }
    }
    // every lane of the block from here on (lanes past the end and outliers carry zeros)
    block_row_sums<CA_FIELDS, NKSR_ICP_FIELDS>(term, partials);
}

extern "C" int nksr_pose_score(const float* src, const float* tgt, int64_t n_pairs, const double* transforms, int64_t n_hyp, double threshold,
                               int32_t* counts_out, void* stream) {
    return hypothesis_score<PoseModel>("pose score", {src, tgt}, n_pairs, transforms, n_hyp, threshold, threshold * threshold, counts_out, stream);
}

extern "C" int nksr_corr_accumulate(const float* src, const float* tgt, int64_t n_pairs, const double* transform, const double* centre,
                                    double threshold, uint8_t* mask_out, double* partials_out, void* stream) {
    if (int rc = threshold_args("corr accumulate", "n_pairs", n_pairs, threshold)) return rc;
    if (n_pairs == 0) return NKSR_OK;
    if (!src || !tgt || !transform || !centre || !mask_out || !partials_out) return nksr_set_error(NKSR_ERR_ARG, "corr accumulate: NULL arrays");
    hipLaunchKernelGGL(k_corr_accumulate, dim3(nksr_blocks(n_pairs, NKSR_ICP_BLOCK)), dim3(NKSR_ICP_BLOCK), 0, (hipStream_t)stream, src, tgt,
                       n_pairs, transform, centre, threshold * threshold, mask_out, partials_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
