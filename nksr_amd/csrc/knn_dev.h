// The single-grid pieces of the neighbour search that more than one file needs (knn.hip, register.hip): the grid as the kernels take
// it, the cell of a query, the fixed-rounding squared distance, and the host-side assembly / checks of the grid arguments.
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
