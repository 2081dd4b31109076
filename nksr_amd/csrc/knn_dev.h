// The single-grid pieces of the neighbour search that more than one file needs (the knn_*.hip files, metrics.hip, register.hip): the
// grid as the kernels take it, the cell of a query, the fixed-rounding squared distance, the candidate scan (knn_cells27, knn_scan4),
// and the host-side assembly / checks of the grid arguments.
#pragma once
#include "common.h"

struct KnnGrid {
    const float* xyz;          // [N,3] Morton-sorted points
    const int32_t* start;      // [ncell] point range of every occupied cell
    const int32_t* end;
    const int64_t* hkeys;      // hash: cell key -> cell index
    const int32_t* hvals;
    int hcap;
    float inv_cell;            // fp32 1 / cell size
    float cell;
};

__device__ __forceinline__ void cell_of(const KnnGrid& g, const float q[3], int c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float p;
        c[a] = half_index(q[a], g.inv_cell, p) >> 1;
    }
}

// squared length with a FIXED rounding sequence: the bisection (count_within) and the later visits of the same candidates must
// agree on every bit of it.  Left to the compiler (device code contracts a*b+c into fmas, and __fmul_rn / __fadd_rn are plain
// operators in HIP) one inlined site fused and the other did not: a neighbour AT the k-th distance was counted but not visited
// (2 - 10 % of the queries of k_sdf_from_points with large cells).  Explicit fmas cannot be re-associated.
__device__ __forceinline__ float knn_d2(float ex, float ey, float ez) {
    return fmaf(ez, ez, fmaf(ey, ey, ex * ex));
}

// The occupied cells among the 27 around cell c, in the order j = 0 .. 26 with offsets (j / 9 - 1, (j / 3) % 3 - 1, j % 3 - 1): f(ci)
// gets the cell's index (its points are start[ci] .. end[ci]) and returns false to end the walk.  For a grid with cell >= radius
// nothing within the radius of a point of cell c lies outside them.
template <class F>
__device__ __forceinline__ void knn_cells27(const KnnGrid& g, const int c[3], F&& f) {
    for (int j = 0; j < 27; ++j) {
        const int ci = hash_find(g.hkeys, g.hvals, g.hcap, morton_biased(c[0] + j / 9 - 1, c[1] + (j / 3) % 3 - 1, c[2] + j % 3 - 1, NKSR_BIAS0));
        if (ci < 0) continue;
        if (!f(ci)) return;
    }
}

// Candidates [s, e) of the sorted cloud handed to f(index, d2), d2 = knn_d2(p - q), ascending and four at a time: the twelve coordinate
// loads of a group are in flight together (one at a time, a cell of 30 points was 30 memory latencies end to end -- a consumer such as
// the sorted insertion needs each distance before the next), then a one-at-a-time tail.  more() is asked before every group and once
// before the tail: a caller that has enough stops there, at most the rest of a group late.  Offsets into xyz are 64-bit: good for
// every cloud whose point ranges fit the int32 start / end arrays.
struct KnnScanAll {
    __device__ __forceinline__ bool operator()() const { return true; }
};
template <class F, class More = KnnScanAll>
__device__ __forceinline__ void knn_scan4(const float* __restrict__ xyz, int s, int e, const float q[3], F&& f, More&& more = More()) {
    int kk = s;
    for (; kk + 4 <= e && more(); kk += 4) {
        float p[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) p[t] = xyz[(int64_t)kk * 3 + t];
#pragma unroll
        for (int t = 0; t < 4; ++t) f(kk + t, knn_d2(p[3 * t] - q[0], p[3 * t + 1] - q[1], p[3 * t + 2] - q[2]));
    }
    if (!more()) return;
    for (; kk < e; ++kk)
        f(kk, knn_d2(xyz[(int64_t)kk * 3] - q[0], xyz[(int64_t)kk * 3 + 1] - q[1], xyz[(int64_t)kk * 3 + 2] - q[2]));
}

static KnnGrid make_grid(const float* xyz_sorted, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                         const int32_t* hvals, int hcap, float cell, float inv_cell) {
    KnnGrid g;
    g.xyz = xyz_sorted; g.start = start; g.end = end; g.hkeys = hkeys; g.hvals = hvals; g.hcap = hcap;
    g.cell = cell;
    g.inv_cell = inv_cell;   // the SAME fp32 reciprocal the host binned the points with
    return g;
}

static int knn_grid_args(const char* who, const float* xyz_sorted, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                         const int32_t* hvals, int32_t hcap, float cell, float inv_cell) {
    if (!xyz_sorted || !start || !end || !hkeys || !hvals) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL grid arrays", who);
    if (hcap < 8 || (hcap & (hcap - 1))) return nksr_set_error(NKSR_ERR_ARG, "%s: hcap must be a power of two >= 8 (got %d)", who, hcap);
    if (!(cell > 0.f) || !(inv_cell > 0.f)) return nksr_set_error(NKSR_ERR_ARG, "%s: cell and inv_cell must be > 0", who);
    return NKSR_OK;
}

// a search within `radius` on the 27 cells of a grid: the radius, the grid, and a cell that covers the radius.  `empty`: the caller has
// nothing to search for and returns after its own checks -- the grid is not looked at
static int radius_grid_args(const char* who, const float* xyz_sorted, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                            const int32_t* hvals, int32_t hcap, float cell, float inv_cell, float radius, bool empty = false) {
    if (!(radius > 0.f) || !(radius < 3.4e38f)) return nksr_set_error(NKSR_ERR_ARG, "%s: radius must be positive and finite", who);
    if (empty) return NKSR_OK;
    if (int rc = knn_grid_args(who, xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell)) return rc;
    if (!(cell >= radius)) return nksr_set_error(NKSR_ERR_ARG, "%s: the grid's cell (%g) must be >= radius (%g)", who, (double)cell, (double)radius);
    return NKSR_OK;
}
