// ext.sdfgen over a Morton-sorted cloud (nksr_amd/neighbours.py: PointGrid, PointPyramid): the estimators and the kernels of both searches.
//
//      k_sdf_from_points, k_knn_mean_dist      nksr_sdf_from_points, nksr_knn_mean_dist (ext.sdfgen with nb_points > 32, on plain grids;
//                                              the block walk and the bisection: knn_walk_dev.h)
//   2. The two estimators of ext.sdfgen.sdf_from_points (SdfVote, SdfImls; reference ext/sdfgen/sdf_from_points.cu:32-140, call sites
//      models/loss.py:85, dataset/av_gt_geometry.py:72), each stated once and fed by both searches.
//   4. (The octree: knn_topk_dev.h.)  On it k_sdf_pyramid (nksr_sdf_from_points_pyramid),
//      k_knn_mean_dist_pyramid (nksr_knn_mean_dist_pyramid: the adaptive_knn radius of ext.sdfgen).
// Queries run in Morton order where they are the cloud itself: neighbouring lanes scan the same cells.
#include "common.h"
#include "knn_walk_dev.h"
#include "knn_topk_dev.h"

// ---- ext.sdfgen.sdf_from_points: the two estimators ---------------------------------------------------------------------------
// Each over the k nearest reference points of a query x, stated once and fed by both searches: by knn_visit in walk order
// (k_sdf_from_points, which finds the nearest neighbour by a running minimum) and from the TopK list nearest first (sdf_estimate,
// whose nearest neighbour is the first occupied slot).  add() takes neighbour kk at offset e = x - p_kk, squared distance d2.
//   vote (ComputeSDFKernel, sdf_from_points.cu:83-140): the nearest neighbour decides the magnitude -- |n.(x-p)| if x lies within
//        stdv * ref_std[p] of it, else |x-p| -- and the majority of sign(n_k.(x-p_k)) over the k neighbours the sign
//        (positive needs MORE than k/2 votes);
//   IMLS (ComputeIMLSKernel, :32-81): sum_k w_k n_k.(x-p_k) / sum_k w_k,  w_k = exp(-(|x-p_k|^2 - min_j |x-p_j|^2) / stdv^2).
// n . e with a FIXED rounding sequence, like knn_d2: two products, their sum, one fma.  The vote's value IS this number (|n.(x-p)| of
// the nearest neighbour); left to the compiler, every kernel it is inlined into picked its own contraction of nx*ex + ny*ey + nz*ez
// and the same query got another last bit from each of them.  (IMLS sums k weighted terms in an order that differs between the two
// searches anyway, and keeps the plain expression.)
__device__ __forceinline__ float sdf_dot(float nx, float ny, float nz, float ex, float ey, float ez) {
#pragma clang fp contract(off)
    const float s = nx * ex + ny * ey;
    return fmaf(nz, ez, s);
}
struct SdfVote {
    int npos = 0;
    float sd = 0.f, g0[3] = {0.f, 0.f, 0.f};
    // nearest: kk is the nearest neighbour (so far, for a caller that learns it on the way: the last such call stands)
    __device__ __forceinline__ void add(const float* __restrict__ nrm, const float* __restrict__ ref_std, float stdv, int kk, float ex, float ey,
                                        float ez, float d2, bool nearest) {
        const float nx = nrm[kk * 3], ny = nrm[kk * 3 + 1], nz = nrm[kk * 3 + 2];
        const float d = sdf_dot(nx, ny, nz, ex, ey, ez);
        npos += d > 0.f;
        if (nearest) {                            // the nearest neighbour sets the magnitude
            const float len = sqrtf(d2);
            if (len < stdv * (ref_std ? ref_std[kk] : 1.f)) {
                sd = fabsf(d);
                const float sg = d > 0.f ? 1.f : -1.f;
                g0[0] = sg * nx; g0[1] = sg * ny; g0[2] = sg * nz;
            } else {
                sd = len;
                g0[0] = ex / len; g0[1] = ey / len; g0[2] = ez / len;
            }
        }
    }
    __device__ __forceinline__ void finish(int k, int64_t i, float* __restrict__ sdf, float* __restrict__ grad) const {
        const float sg = npos <= k / 2 ? -1.f : 1.f;
        sdf[i] = sg * sd;
        if (grad) { grad[i * 3] = sg * g0[0]; grad[i * 3 + 1] = sg * g0[1]; grad[i * 3 + 2] = sg * g0[2]; }
    }
};
struct SdfImls {
    float inv_s2, emin = 0.f, wsum = 0.f, acc = 0.f, gr[3] = {0.f, 0.f, 0.f};
    __device__ __forceinline__ explicit SdfImls(float stdv) : inv_s2(1.f / (stdv * stdv)) {}
    __device__ __forceinline__ void nearest(float d2min) { emin = d2min * inv_s2; }      // before the first add()
    __device__ __forceinline__ void add(const float* __restrict__ nrm, int kk, float ex, float ey, float ez, float d2) {
        const float nx = nrm[kk * 3], ny = nrm[kk * 3 + 1], nz = nrm[kk * 3 + 2];
        const float w = expf(-d2 * inv_s2 + emin);
        wsum += w;
        acc += (nx * ex + ny * ey + nz * ez) * w;
        gr[0] += nx * w; gr[1] += ny * w; gr[2] += nz * w;
    }
    __device__ __forceinline__ void finish(int64_t i, float* __restrict__ sdf, float* __restrict__ grad) const {
        sdf[i] = acc / wsum;
        if (grad) { grad[i * 3] = gr[0] / wsum; grad[i * 3 + 1] = gr[1] / wsum; grad[i * 3 + 2] = gr[2] / wsum; }
    }
};

// Any k, one grid: knn_radius, then one pass over the neighbour set (vote) or two (IMLS) -- no index lists, no sort.
// valid = 0: fewer than k reference points within max_ring cells (the host retries those queries on a coarser grid).
__global__ void __launch_bounds__(128) k_sdf_from_points(KnnGrid g, const float* __restrict__ nrm, const float* __restrict__ ref_std,
                                                         const float* __restrict__ query, int64_t nq, int k, int max_ring, float stdv,
                                                         int imls, float* __restrict__ sdf, float* __restrict__ grad,
                                                         int32_t* __restrict__ valid) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float q[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
    int c[3], R;
    float r2;
    cell_of(g, q, c);
    if (!knn_radius(g, q, c, k, max_ring, R, r2)) { valid[i] = 0; return; }
    valid[i] = 1;
    float dmin = 3.4e38f;
    if (imls) {
        knn_visit(g, q, c, R, r2, k, [&](int, float, float, float, float d2) { dmin = fminf(dmin, d2); });
        SdfImls est(stdv);
        est.nearest(dmin);
        knn_visit(g, q, c, R, r2, k, [&](int kk, float ex, float ey, float ez, float d2) { est.add(nrm, kk, ex, ey, ez, d2); });
        est.finish(i, sdf, grad);
    } else {
        SdfVote est;
        knn_visit(g, q, c, R, r2, k, [&](int kk, float ex, float ey, float ez, float d2) {
            const bool nearest = d2 < dmin;
            if (nearest) dmin = d2;
            est.add(nrm, ref_std, stdv, kk, ex, ey, ez, d2, nearest);
        });
        est.finish(k, i, sdf, grad);
    }
}

// mean distance of every (sorted) reference point to its k nearest reference points, itself included (the adaptive_knn radius,
// sdf_from_points.cu:176-184)
__global__ void __launch_bounds__(128) k_knn_mean_dist(KnnGrid g, int64_t n, int k, int max_ring, float* __restrict__ out,
                                                       int32_t* __restrict__ valid) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float q[3] = {g.xyz[i * 3], g.xyz[i * 3 + 1], g.xyz[i * 3 + 2]};
    int c[3], R;
    float r2;
    cell_of(g, q, c);
    if (!knn_radius(g, q, c, k, max_ring, R, r2)) { valid[i] = 0; out[i] = 0.f; return; }
    float s = 0.f;
    knn_visit(g, q, c, R, r2, k, [&](int, float, float, float, float d2) { s += sqrtf(d2); });
    out[i] = s / (float)k;
    valid[i] = 1;
}

// the two estimators over the k nearest neighbours in `top`: nearest first, the nearest in slot KMAX - k
template <int KMAX>
__device__ __forceinline__ void sdf_estimate(const float* __restrict__ xyz, const float* __restrict__ nrm, const float* __restrict__ ref_std, const float q[3],
                                             const TopK<KMAX>& top, int k, float stdv, int imls, int64_t i, float* __restrict__ sdf,
                                             float* __restrict__ grad) {
    if (imls) {
        SdfImls est(stdv);
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < KMAX - k) continue;
            if (j == KMAX - k) est.nearest(top.d2[j]);
            const int kk = top.idx[j];
            est.add(nrm, kk, q[0] - xyz[kk * 3], q[1] - xyz[kk * 3 + 1], q[2] - xyz[kk * 3 + 2], top.d2[j]);
        }
        est.finish(i, sdf, grad);
    } else {
        SdfVote est;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < KMAX - k) continue;
            const int kk = top.idx[j];
            est.add(nrm, ref_std, stdv, kk, q[0] - xyz[kk * 3], q[1] - xyz[kk * 3 + 1], q[2] - xyz[kk * 3 + 2], top.d2[j], j == KMAX - k);
        }
        est.finish(k, i, sdf, grad);
    }
}

template <int KMAX>
__global__ void __launch_bounds__(KNN_PYR_BLOCK) k_sdf_pyramid(KnnPyramid Parg, const float* __restrict__ nrm, const float* __restrict__ ref_std,
                                                               const float* __restrict__ query, int64_t nq, int k, int max_ring, float stdv,
                                                               int imls, float* __restrict__ sdf, float* __restrict__ grad,
                                                               int32_t* __restrict__ valid) {
    int* node;
    unsigned char* cursor;
    const KnnPyramid& P = knn_pyramid_lds(Parg, node, cursor);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float q[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
    TopK<KMAX> top;
    if (!knn_topk_pyramid<KMAX>(P, q, k, max_ring, top, node, cursor)) { valid[i] = 0; return; }
    valid[i] = 1;
    sdf_estimate<KMAX>(P.xyz, nrm, ref_std, q, top, k, stdv, imls, i, sdf, grad);
}
template <int KMAX>
__global__ void __launch_bounds__(KNN_PYR_BLOCK) k_knn_mean_dist_pyramid(KnnPyramid Parg, int64_t n, int k, int max_ring, float* __restrict__ out,
                                                                         int32_t* __restrict__ valid) {
    int* node;
    unsigned char* cursor;
    const KnnPyramid& P = knn_pyramid_lds(Parg, node, cursor);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float q[3] = {P.xyz[i * 3], P.xyz[i * 3 + 1], P.xyz[i * 3 + 2]};
    TopK<KMAX> top;
    if (!knn_topk_pyramid<KMAX>(P, q, k, max_ring, top, node, cursor)) { valid[i] = 0; out[i] = 0.f; return; }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j >= KMAX - k) s += sqrtf(top.d2[j]);
    out[i] = s / (float)k;
    valid[i] = 1;
}

extern "C" int nksr_sdf_from_points(const float* xyz_sorted, const float* normal_sorted, const float* ref_std_sorted, const int32_t* start,
                                    const int32_t* end, const int64_t* hkeys, const int32_t* hvals, int32_t hcap, float cell, float inv_cell,
                                    const float* query, int64_t nq, int k, int max_ring, float stdv, int imls, float* sdf_out,
                                    float* grad_out, int32_t* valid_out, void* stream) {
    if (nq <= 0) return NKSR_OK;
    if (k < 1) return nksr_set_error(NKSR_ERR_ARG, "nb_points must be >= 1");
    if (!(stdv > 0.f)) return nksr_set_error(NKSR_ERR_ARG, "stdv must be > 0");
    if (!xyz_sorted || !normal_sorted || !query || !sdf_out || !valid_out) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    hipLaunchKernelGGL(k_sdf_from_points, dim3(nksr_blocks(nq, 128)), dim3(128), 0, (hipStream_t)stream, g, normal_sorted, ref_std_sorted, query,
                       nq, k, max_ring, stdv, imls, sdf_out, grad_out, valid_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_sdf_from_points_pyramid(const nksr_knn_pyramid_t* pyramid, const float* normal_sorted, const float* ref_std_sorted, const float* query,
                                            int64_t nq, int k, int max_ring, float stdv, int imls, float* sdf_out, float* grad_out,
                                            int32_t* valid_out, void* stream) {
    if (nq <= 0) return NKSR_OK;
    if (k < 1 || k > 32) return nksr_set_error(NKSR_ERR_ARG, "pyramid search: 1 <= nb_points <= 32 (got %d)", k);
    if (!(stdv > 0.f)) return nksr_set_error(NKSR_ERR_ARG, "stdv must be > 0");
    if (!normal_sorted || !query || !sdf_out || !valid_out) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    KnnPyramid P;
    if (int rc = make_pyramid(P, pyramid)) return rc;
    KNN_PYR_DISPATCH(k_sdf_pyramid, 32, k, nq, P, normal_sorted, ref_std_sorted, query, nq, k, max_ring, stdv, imls, sdf_out, grad_out, valid_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
extern "C" int nksr_knn_mean_dist_pyramid(const nksr_knn_pyramid_t* pyramid, int64_t n, int k, int max_ring, float* out, int32_t* valid_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (k < 1 || k > 32) return nksr_set_error(NKSR_ERR_ARG, "pyramid search: 1 <= k <= 32 (got %d)", k);
    KnnPyramid P;
    if (int rc = make_pyramid(P, pyramid)) return rc;
    KNN_PYR_DISPATCH(k_knn_mean_dist_pyramid, 32, k, n, P, n, k, max_ring, out, valid_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_knn_mean_dist(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                  const int32_t* hvals, int32_t hcap, float cell, float inv_cell, int k, int max_ring, float* out,
                                  int32_t* valid_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (k < 1) return nksr_set_error(NKSR_ERR_ARG, "k must be >= 1");
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    hipLaunchKernelGGL(k_knn_mean_dist, dim3(nksr_blocks(n, 128)), dim3(128), 0, (hipStream_t)stream, g, n, k, max_ring, out, valid_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
