// Point-cloud segmentation (nksr_amd/segment.py: cloud.cluster_dbscan, cloud.segment_plane, cloud.plane_scores).
//
// A. DBSCAN on a PointGrid whose cell is >= eps (CloudIndex._radius_grid).  THE DEFINITION the kernels are held to:
//      neighbours   j is a neighbour of i iff knn_d2(x_j - x_i) <= fl32(eps) * fl32(eps): the fp32 predicate of k_radius_count (r2 is
//                   formed from the fp32 radius on the host side of the entry point, as there), inclusive; a point is its own neighbour
//      core         a point with at least min_points neighbours, itself included: nksr_radius_count(cap = min_points, exclude_self = 0)
//                   as it is -- the flags come in as an array, there is no second statement of the predicate for them
//      clusters     two core points that are neighbours are in one cluster; clusters = the connected components of that graph
//      border       a non-core point with at least one core neighbour takes the LOWEST LABEL among its core neighbours; every other
//                   non-core point is noise (-1)
//      label order  0 .. C - 1 in ascending order of the smallest CALLER index among each cluster's core points
//    k_dbscan_hook        one lane per sorted point, core lanes only: the 27 cells (knn_cells27 / knn_scan4), every core neighbour
//                         j < i hooked as uf_hook does (uf_dev.h, whose determinism argument holds verbatim: the roots end as the
//                         minimum SORTED index of every component).  The lane caches its current root and skips the find when
//                         parent[j] already equals it (parent[j] lies in j's set, the cached root in i's: equal means joined).
//                         Two passes: <true> hooks the FIRST core neighbour j < i alone (a capped walk), k_dbscan_shorten points
//                         every node at its root, and <false>, the pass over every pair, then finds most pairs joined already and
//                         skips them at the cost of one load.  The first pass hooks a subset of the pairs of the second, so the
//                         result is that of the second alone; measured against it in profiles/segment.md (1.3 - 1.5 x faster).
//    k_dbscan_min_caller  min over a component's points of perm (sorted -> caller index) into min_index[root]: integer atomicMin, one
//                         per wavefront and root, so the result does not depend on the lane order; the host ranks the roots by it
//    k_dbscan_border      after the core labels exist: the same walk for non-core lanes, the minimum label over core neighbours
//    Integers only: every array repeats bit for bit.
//
// B. Plane RANSAC.  Residual of point (x, y, z) (fp32, widened) to plane (a, b, c, d): s = ((a x + b y) + c z) + d in fp64, every
//    product and sum rounded on its own (no fused multiply-add); inlier iff |s| <= t.
//    PlaneModel       nksr_plane_score: all H hypotheses in one launch of k_hypothesis_score (score_dev.h), integer counts.
//                     A hypothesis that is not finite or whose normal is zero is degenerate: its count is -1.
//    k_plane_moments  the inlier mask of ONE plane and, per workgroup, the fp64 sums of 1, x'_a and x'_a x'_b (a <= b) over the inliers,
//                     x' = x - centre: rows NKSR_ICP_FIELDS wide, reduced in the fixed order of block_row_sums (icp_dev.h; then
//                     nksr_icp_reduce over the rows).  No atomics.
#include "common.h"
#include "icp_dev.h"
#include "knn_dev.h"
#include "score_dev.h"
#include "uf_dev.h"
#include "wave_dev.h"

#define DB_BLOCK 128

// ---- A. DBSCAN ---------------------------------------------------------------------------------------------------------------------
// FIRST: the lane hooks the first core neighbour j < i it meets and ends its walk; else every core neighbour j < i.
template <bool FIRST>
__global__ void __launch_bounds__(DB_BLOCK) k_dbscan_hook(KnnGrid g, int64_t n, float r2, const uint8_t* __restrict__ core, int32_t* parent) {
    const int64_t i64 = (int64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (i64 >= n || !core[i64]) return;
    const int i = (int)i64;
    const float q[3] = {g.xyz[i64 * 3], g.xyz[i64 * 3 + 1], g.xyz[i64 * 3 + 2]};
    int c[3];
    cell_of(g, q, c);
    int32_t root = FIRST ? i : uf_load(parent + i);     // what the lane last saw as the root of its set (an ancestor of i at all times)
    bool done = false;
    auto more = [&]() { return !done; };
    knn_cells27(g, c, [&](int ci) {
        const int s = g.start[ci], e = g.end[ci] < i ? g.end[ci] : i;          // every pair once: j < i
        knn_scan4(g.xyz, s, e, q, [&](int j, float d2) {
            if (FIRST) {
                if (!done && d2 <= r2 && core[j]) { uf_hook(parent, i, j); done = true; }
            } else if (d2 <= r2 && core[j] && uf_load(parent + j) != root) {
                root = uf_hook(parent, root, j);
            }
        }, more);
        return !done;
    });
}

// parent[i] = the root of i, no flags (between the two hook passes)
__global__ void __launch_bounds__(UF_BLOCK) k_dbscan_shorten(int32_t* parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * UF_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t r = uf_load(parent + i);
    if (r < 0) return;
    while (true) {
        const int32_t p = uf_load(parent + r);
        if (p == r) break;
        r = p;
    }
    if (r != (int32_t)i) uf_store(parent + i, r);
}

__global__ void __launch_bounds__(UF_BLOCK) k_dbscan_min_caller(const int32_t* __restrict__ parent, const int64_t* __restrict__ perm, int64_t n,
                                                                int32_t* min_index) {
    const int64_t i = (int64_t)blockIdx.x * UF_BLOCK + threadIdx.x;
    const int32_t r = i < n ? parent[i] : -1;
    const bool active = r >= 0;
    const int32_t mine = active ? (int32_t)perm[i] : 0x7FFFFFFF;
    const int lane = threadIdx.x & (NKSR_WAVE - 1);
    unsigned long long todo = __ballot(active);         // (every lane of the wavefront stays in the loop: the shuffles need them)
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t r0 = __shfl(r, leader);
        const bool in_group = active && r == r0;
        int32_t m = in_group ? mine : 0x7FFFFFFF;
#pragma unroll
        for (int o = NKSR_WAVE / 2; o > 0; o >>= 1) {
            const int32_t other = __shfl_xor(m, o);
            m = other < m ? other : m;
        }
        if (lane == leader) atomicMin(min_index + r0, m);
        todo &= ~__ballot(in_group);
    }
}

__global__ void __launch_bounds__(DB_BLOCK) k_dbscan_border(KnnGrid g, int64_t n, float r2, const uint8_t* __restrict__ core, int32_t* label) {
    const int64_t i = (int64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (i >= n || core[i]) return;                      // (core lanes keep their label; non-core lanes read core labels only)
    const float q[3] = {g.xyz[i * 3], g.xyz[i * 3 + 1], g.xyz[i * 3 + 2]};
    int c[3];
    cell_of(g, q, c);
    int32_t best = 0x7FFFFFFF;
    knn_cells27(g, c, [&](int ci) {
        knn_scan4(g.xyz, g.start[ci], g.end[ci], q, [&](int j, float d2) {
            if (d2 <= r2 && core[j]) {
                const int32_t l = label[j];
                best = l < best ? l : best;
            }
        });
        return true;
    });
    label[i] = best == 0x7FFFFFFF ? -1 : best;
}

static int dbscan_args(const char* who, const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                       const int32_t* hvals, int32_t hcap, float cell, float inv_cell, float radius) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: n=%lld outside [0, 2^31)", who, (long long)n);
    return radius_grid_args(who, xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell, radius, n == 0);
}

extern "C" int nksr_dbscan_components(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                      const int32_t* hvals, int32_t hcap, float cell, float inv_cell, float radius, const uint8_t* core,
                                      int32_t* parent_out, int32_t* root_flags_out, void* stream) {
    if (int rc = dbscan_args("dbscan components", xyz_sorted, n, start, end, hkeys, hvals, hcap, cell, inv_cell, radius)) return rc;
    if (!root_flags_out || (n > 0 && (!core || !parent_out))) return nksr_set_error(NKSR_ERR_ARG, "dbscan components: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { NKSR_CHECK_HIP(hipMemsetAsync(root_flags_out, 0, sizeof(int32_t), st)); return NKSR_OK; }
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    UF_LAUNCH(k_uf_init, n, st, parent_out, n, core);
    const dim3 grid(nksr_blocks(n, DB_BLOCK)), block(DB_BLOCK);
    hipLaunchKernelGGL(k_dbscan_hook<true>, grid, block, 0, st, g, n, radius * radius, core, parent_out);
    NKSR_CHECK_LAUNCH();
    UF_LAUNCH(k_dbscan_shorten, n, st, parent_out, n);
    hipLaunchKernelGGL(k_dbscan_hook<false>, grid, block, 0, st, g, n, radius * radius, core, parent_out);
    NKSR_CHECK_LAUNCH();
    UF_LAUNCH(k_uf_flatten, n, st, parent_out, n, root_flags_out);
    return NKSR_OK;
}

extern "C" int nksr_dbscan_min_caller(const int32_t* parent, const int64_t* perm, int64_t n, int32_t* min_index_out, void* stream) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "dbscan min caller: n=%lld outside [0, 2^31)", (long long)n);
    if (n == 0) return NKSR_OK;
    if (!parent || !perm || !min_index_out) return nksr_set_error(NKSR_ERR_ARG, "dbscan min caller: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(min_index_out, 0x7F, sizeof(int32_t) * (size_t)n, st));
    UF_LAUNCH(k_dbscan_min_caller, n, st, parent, perm, n, min_index_out);
    return NKSR_OK;
}

extern "C" int nksr_dbscan_border(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                  const int32_t* hvals, int32_t hcap, float cell, float inv_cell, float radius, const uint8_t* core,
                                  int32_t* label, void* stream) {
    if (int rc = dbscan_args("dbscan border", xyz_sorted, n, start, end, hkeys, hvals, hcap, cell, inv_cell, radius)) return rc;
    if (n == 0) return NKSR_OK;
    if (!core || !label) return nksr_set_error(NKSR_ERR_ARG, "dbscan border: NULL arrays");
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    hipLaunchKernelGGL(k_dbscan_border, dim3(nksr_blocks(n, DB_BLOCK)), dim3(DB_BLOCK), 0, (hipStream_t)stream, g, n, radius * radius, core, label);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// ---- B. plane RANSAC ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double plane_residual(const double* __restrict__ p, double x, double y, double z) {
#pragma clang fp contract(off)
    const double u = p[0] * x + p[1] * y;
    const double v = u + p[2] * z;
    return v + p[3];
}
__device__ __forceinline__ bool plane_degenerate(const double* __restrict__ p) {
    const bool finite = fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY && fabs(p[3]) < INFINITY;       // (false for a NaN)
    return !finite || (p[0] == 0.0 && p[1] == 0.0 && p[2] == 0.0);
}

// the model of k_hypothesis_score (score_dev.h): 4 points a lane (12 doubles), 128 planes a workgroup (4 KB, and 2 KB of counts)
struct PlaneModel {
    static constexpr int WIDTH = 4, ITEMS = 4, CHUNK = 128, MAX_H = 1 << 20;
    static constexpr const char* N_NAME = "n";
    static constexpr const char* H_NAME = "n_planes";
    struct Items {
        const float* __restrict__ xyz;
        bool missing() const { return !xyz; }
    };
    struct Item { double x, y, z; };
    static __device__ __forceinline__ void load(const Items& in, int64_t i, bool on, Item& p) {
        p.x = on ? (double)in.xyz[i * 3] : (double)NAN;           // a lane past the end carries a NaN: no comparison with it holds
        p.y = on ? (double)in.xyz[i * 3 + 1] : (double)NAN;
        p.z = on ? (double)in.xyz[i * 3 + 2] : (double)NAN;
    }
    static __device__ __forceinline__ bool inlier(const double* plane, const Item& p, double t) {
        return fabs(plane_residual(plane, p.x, p.y, p.z)) <= t;
    }
    static __device__ __forceinline__ bool degenerate(const double* plane) { return plane_degenerate(plane); }
};

static_assert(NKSR_PLANE_MOMENT + 6 == NKSR_PLANE_FIELDS && NKSR_PLANE_FIELDS <= NKSR_ICP_FIELDS,
              "layout of the sums inside a row nksr_icp_reduce takes");

__global__ void __launch_bounds__(NKSR_ICP_BLOCK) k_plane_moments(const float* __restrict__ xyz, int64_t n, const double* __restrict__ plane,
                                                                  const double* __restrict__ centre, double t, uint8_t* __restrict__ mask,
                                                                  double* __restrict__ partials) {
    const int64_t i = (int64_t)blockIdx.x * NKSR_ICP_BLOCK + threadIdx.x;
    double term[NKSR_PLANE_FIELDS];
#pragma unroll
    for (int f = 0; f < NKSR_PLANE_FIELDS; ++f) term[f] = 0.0;
    if (i < n) {
        const double p[3] = {(double)xyz[i * 3], (double)xyz[i * 3 + 1], (double)xyz[i * 3 + 2]};
        const bool in = fabs(plane_residual(plane, p[0], p[1], p[2])) <= t;
        mask[i] = in ? 1 : 0;
        if (in) {
#pragma clang fp contract(off)
            const double d[3] = {p[0] - centre[0], p[1] - centre[1], p[2] - centre[2]};
            term[NKSR_PLANE_COUNT] = 1.0;
            int k = NKSR_PLANE_MOMENT;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                term[NKSR_PLANE_SUM + a] = d[a];
#pragma unroll
                for (int b = a; b < 3; ++b) term[k++] = d[a] * d[b];
            }
        }
    }
    // every lane of the block from here on (lanes past the end and outliers carry zeros)
    block_row_sums<NKSR_PLANE_FIELDS>(term, partials);
}

extern "C" int nksr_plane_score(const float* xyz, int64_t n, const double* planes, int64_t n_planes, double threshold, int32_t* counts_out,
                                void* stream) {
    return hypothesis_score<PlaneModel>("plane score", {xyz}, n, planes, n_planes, threshold, threshold, counts_out, stream);
}

extern "C" int nksr_plane_moments(const float* xyz, int64_t n, const double* plane, const double* centre, double threshold, uint8_t* mask_out,
                                  double* partials_out, void* stream) {
    if (int rc = threshold_args("plane moments", "n", n, threshold)) return rc;
    if (n == 0) return NKSR_OK;
    if (!xyz || !plane || !centre || !mask_out || !partials_out) return nksr_set_error(NKSR_ERR_ARG, "plane moments: NULL arrays");
    hipLaunchKernelGGL(k_plane_moments, dim3(nksr_blocks(n, NKSR_ICP_BLOCK)), dim3(NKSR_ICP_BLOCK), 0, (hipStream_t)stream, xyz, n, plane, centre,
                       threshold, mask_out, partials_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
