// Queries over a Morton-sorted cloud (nksr_amd/neighbours.py: PointGrid, PointPyramid) that hand the neighbours themselves back.
//
//      k_nearest_index    nksr_nearest_index (PointGrid.nearest: the colour lookup of fields.PCNNField; the block walk: knn_walk_dev.h)
//   4. (The octree: knn_topk_dev.h.)  k_pyramid_level (nksr_knn_pyramid_level builds a level).
//   5. Query kernels: k_knn_query_pyramid (nksr_knn_query_pyramid, nksr_amd/cloud.py and orient.py: the k
//      nearest written out), k_radius_count (nksr_radius_count: the 27 cells of a grid with cell >= radius).
// Queries run in Morton order where they are the cloud itself: neighbouring lanes scan the same cells.
#include "common.h"
#include "knn_walk_dev.h"
#include "knn_topk_dev.h"

__global__ void __launch_bounds__(128) k_nearest_index(KnnGrid g, const float* __restrict__ query, int64_t nq, int max_ring,
                                                       int32_t* __restrict__ index) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float q[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
    int c[3];
    cell_of(g, q, c);
    int best = -1;
    float bd = 3.4e38f;
    for (int R = 1; R <= max_ring; ++R) {
        // scan the shell |offset|_inf == R (R = 1: the full 3^3 block)
        knn_block<true>(g, q, c, R, [&](int k, float, float, float, float d) {
            if (d < bd || (d == bd && k < best)) { bd = d; best = k; }
        });
        // everything closer than R*cell has been seen
        const float rr = (float)R * g.cell;
        if (best >= 0 && bd <= rr * rr) break;
    }
    index[i] = best;
}

// one level of the octree from the one below: thread p owns parent cell p (keys = sorted unique child keys >> 3)
__global__ void __launch_bounds__(256) k_pyramid_level(const int64_t* __restrict__ ckeys, int32_t nc, const int32_t* __restrict__ cstart,
                                                       const int32_t* __restrict__ cend, const int64_t* __restrict__ pkeys, int32_t np,
                                                       int32_t* __restrict__ child, uint8_t* __restrict__ cmask, int32_t* __restrict__ pstart,
                                                       int32_t* __restrict__ pend) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int64_t key = pkeys[p];
    int lo = 0, hi = nc;                                    // first child: lower bound of key << 3
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((ckeys[mid] >> 3) < key) lo = mid + 1; else hi = mid;
    }
    unsigned m = 0u;
    int j = lo;
    for (; j < nc && (ckeys[j] >> 3) == key; ++j) m |= 1u << (unsigned)(ckeys[j] & 7);
    child[p] = lo;
    if (p == np - 1) child[np] = nc;
    cmask[p] = (uint8_t)m;
    pstart[p] = cstart[lo];
    pend[p] = cend[j - 1];
}

// ---- the k nearest WRITTEN OUT, and the points within a radius counted (nksr_amd/cloud.py) ---------------------------------------------
// The search is knn_topk_pyramid (one thread per query, the block shape and LDS stacks of k_sdf_pyramid);
// the new work is the stores.  exclude_self: the list is searched with one slot more (kk = k + 1) and the query's own point dropped
// from it on the way out -- it is the nearest candidate or tied with it at distance 0, so it is in the list unless kk OTHER points
// lie at distance 0 too, and then the first k of the list are k nearest others all the same.  Points that merely share the
// position stay.  (kk = 33 takes a list of its own size: TopK<33>.)
template <int KMAX>
__device__ __forceinline__ void knn_write(const TopK<KMAX>& top, int kk, int k, int self, int64_t i, int32_t* __restrict__ idx_out,
                                          float* __restrict__ d2_out) {
    int w = 0;
    bool skip = self >= 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < KMAX - kk) continue;
        if (skip && top.idx[j] == self) { skip = false; continue; }
        if (w < k) {
            idx_out[i * k + w] = top.idx[j];
            d2_out[i * k + w] = top.d2[j];
            ++w;
        }
    }
}
template <int KMAX>
__global__ void __launch_bounds__(KNN_PYR_BLOCK) k_knn_query_pyramid(KnnPyramid Parg, const float* __restrict__ query, int64_t nq, int k, int exclude_self,
                                                                     const int32_t* __restrict__ self_index, int max_ring,
                                                                     int32_t* __restrict__ idx_out, float* __restrict__ d2_out,
                                                                     int32_t* __restrict__ valid) {
    int* node;
    unsigned char* cursor;
    const KnnPyramid& P = knn_pyramid_lds(Parg, node, cursor);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float* qp = query ? query + i * 3 : P.xyz + i * 3;
    const float q[3] = {qp[0], qp[1], qp[2]};
    const int kk = k + (exclude_self ? 1 : 0);
    TopK<KMAX> top;
    if (!knn_topk_pyramid<KMAX>(P, q, kk, max_ring, top, node, cursor)) { valid[i] = 0; return; }
    valid[i] = 1;
    knn_write<KMAX>(top, kk, k, exclude_self ? (self_index ? self_index[i] : (int)i) : -1, i, idx_out, d2_out);
}
// One thread per query, the 27 cells around it (cell >= radius: nothing within the radius lies outside them).  The count may pass
// `cap` by the rest of a group of four before the scan stops: clamped at the end.
__global__ void __launch_bounds__(128) k_radius_count(KnnGrid g, const float* __restrict__ query, int64_t nq, float r2, int cap, int exclude_self,
                                                      const int32_t* __restrict__ self_index, int32_t* __restrict__ count) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float* qp = query ? query + i * 3 : g.xyz + i * 3;
    const float q[3] = {qp[0], qp[1], qp[2]};
    const int self = exclude_self ? (self_index ? self_index[i] : (int)i) : -1;
    int c[3];
    cell_of(g, q, c);
    int n = 0;
    auto more = [&]() { return n < cap; };
    knn_cells27(g, c, [&](int ci) {
        knn_scan4(g.xyz, g.start[ci], g.end[ci], q, [&](int kk, float d2) { n += kk != self && d2 <= r2; }, more);
        return more();
    });
    count[i] = n < cap ? n : cap;
}

extern "C" int nksr_nearest_index(const float* xyz_sorted, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                  const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const float* query, int64_t nq, int max_ring,
                                  int32_t* index_out, void* stream) {
    if (nq <= 0) return NKSR_OK;
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    hipLaunchKernelGGL(k_nearest_index, dim3(nksr_blocks(nq, 128)), dim3(128), 0, (hipStream_t)stream, g, query, nq, max_ring,
                       index_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_knn_pyramid_level(const int64_t* child_keys, int32_t n_child, const int32_t* child_start, const int32_t* child_end,
                                      const int64_t* keys, int32_t n, int32_t* child_out, uint8_t* cmask_out, int32_t* start_out,
                                      int32_t* end_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!child_keys || !child_start || !child_end || !keys || !child_out || !cmask_out || !start_out || !end_out || n_child < n)
        return nksr_set_error(NKSR_ERR_ARG, "kNN pyramid level: NULL arrays or more parents than children");
    hipLaunchKernelGGL(k_pyramid_level, dim3(nksr_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, child_keys, n_child, child_start, child_end,
                       keys, n, child_out, cmask_out, start_out, end_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

static int knn_query_args(const char* who, int64_t n_ref, const float* query, int64_t nq, int k, int exclude_self, int max_ring,
                          const void* idx_out, const void* d2_out, const void* valid_out) {
    if (nq < 0 || n_ref < 0) return nksr_set_error(NKSR_ERR_ARG, "%s: negative size (nq=%lld, n_ref=%lld)", who, (long long)nq, (long long)n_ref);
    if (k < 1 || k > 32) return nksr_set_error(NKSR_ERR_ARG, "%s: 1 <= k <= 32 (got %d)", who, k);
    if (k + (exclude_self ? 1 : 0) > n_ref)
        return nksr_set_error(NKSR_ERR_ARG, "%s: k = %d%s of %lld reference points", who, k, exclude_self ? " others" : "", (long long)n_ref);
    if (!query && nq > n_ref) return nksr_set_error(NKSR_ERR_ARG, "%s: query NULL (the cloud itself) with nq = %lld > n_ref = %lld", who, (long long)nq, (long long)n_ref);
    if (max_ring < 1) return nksr_set_error(NKSR_ERR_ARG, "%s: max_ring must be >= 1 (got %d)", who, max_ring);
    if (nq > 0 && (!idx_out || !d2_out || !valid_out)) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL output arrays", who);
    return NKSR_OK;
}
extern "C" int nksr_knn_query_pyramid(const nksr_knn_pyramid_t* pyramid, int64_t n_ref, const float* query, int64_t nq, int k, int exclude_self,
                                      const int32_t* self_index, int max_ring, int32_t* idx_out, float* dist2_out, int32_t* valid_out, void* stream) {
    if (int rc = knn_query_args("knn query (pyramid)", n_ref, query, nq, k, exclude_self, max_ring, idx_out, dist2_out, valid_out)) return rc;
    KnnPyramid P;
    if (int rc = make_pyramid(P, pyramid)) return rc;
    if (nq == 0) return NKSR_OK;
    KNN_PYR_DISPATCH(k_knn_query_pyramid, 33, k + (exclude_self ? 1 : 0), nq, P, query, nq, k, exclude_self, self_index, max_ring, idx_out, dist2_out,
                     valid_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
extern "C" int nksr_radius_count(const float* xyz_sorted, int64_t n_ref, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                 const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const float* query, int64_t nq, float radius,
                                 int32_t cap, int exclude_self, const int32_t* self_index, int32_t* count_out, void* stream) {
    if (nq < 0 || n_ref < 0) return nksr_set_error(NKSR_ERR_ARG, "radius count: negative size (nq=%lld, n_ref=%lld)", (long long)nq, (long long)n_ref);
    if (int rc = radius_grid_args("radius count", xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell, radius)) return rc;
    if (!query && nq > n_ref) return nksr_set_error(NKSR_ERR_ARG, "radius count: query NULL (the cloud itself) with nq = %lld > n_ref = %lld", (long long)nq, (long long)n_ref);
    if (nq > 0 && !count_out) return nksr_set_error(NKSR_ERR_ARG, "radius count: NULL output array");
    if (nq == 0) return NKSR_OK;
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    hipLaunchKernelGGL(k_radius_count, dim3(nksr_blocks(nq, 128)), dim3(128), 0, (hipStream_t)stream, g, query, nq, radius * radius,
                       cap > 0 ? (int)cap : 0x7fffffff, exclude_self, self_index, count_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
