// Neighbour search over a Morton-sorted cloud (nksr_amd/neighbours.py: PointGrid = the sorted points, the point range of every
// occupied cell and the cell hash; PointPyramid = an octree of such levels over the same points).  What is in this file:
//
//   1. One grid, any k: the block walk and the bisection.
//        knn_block        the cells c + [-R, R]^3 in a fixed order, every candidate handed to a visitor with knn_d2 of its offset
//        knn_radius       smallest ring whose inscribed ball holds k points, then the EXACT k-th smallest squared distance by a 32-step
//                         bisection on the float bit pattern (positive floats order like their bit patterns), each step re-counting
//                         the block (L1/L2 resident): exact selection without a per-thread heap
//        knn_visit        the k neighbours that radius defines, in walk order
// Used by knn_normals.hip (k_knn_pca_normals), knn_sdf.hip (k_sdf_from_points, k_knn_mean_dist) and knn_query.hip (k_nearest_index).
#pragma once
#include "common.h"
#include "knn_dev.h"

// The (2R+1)^3 block of cells around cell c, walked in ONE order -- dx outer, dz inner, the points of a cell ascending -- and every
// candidate p handed to f(index, ex, ey, ez, d2): e = q - p (the sign the estimators take it in), d2 = knn_d2(e).  The order is part
// of the contract: the tie rule of knn_visit, the index tie-break of k_nearest_index and the fp64 sums of the normals depend on it.
// SHELL: for R > 1 only the cells with |offset|_inf == R (the rings inside were walked before).
template <bool SHELL = false, class F>
__device__ __forceinline__ void knn_block(const KnnGrid& g, const float q[3], const int c[3], int R, F&& f) {
    for (int dx = -R; dx <= R; ++dx)
        for (int dy = -R; dy <= R; ++dy)
            for (int dz = -R; dz <= R; ++dz) {
                if (SHELL && R > 1 && abs(dx) < R && abs(dy) < R && abs(dz) < R) continue;
                const int ci = hash_find(g.hkeys, g.hvals, g.hcap, morton_biased(c[0] + dx, c[1] + dy, c[2] + dz, NKSR_BIAS0));
                if (ci < 0) continue;
                for (int k = g.start[ci]; k < g.end[ci]; ++k) {
                    const float ex = q[0] - g.xyz[k * 3], ey = q[1] - g.xyz[k * 3 + 1], ez = q[2] - g.xyz[k * 3 + 2];
                    f(k, ex, ey, ez, knn_d2(ex, ey, ez));
                }
            }
}

// number of candidates with squared distance <= r2 inside the (2R+1)^3 block around cell c
__device__ __forceinline__ int count_within(const KnnGrid& g, const float q[3], const int c[3], int R, float r2) {
    int n = 0;
    knn_block(g, q, c, R, [&](int, float, float, float, float d2) { n += d2 <= r2; });
    return n;
}

// smallest ring R whose inscribed ball already holds k points (then the k nearest are inside its block), and r2 = the exact k-th
// smallest squared distance: bisection on the bit pattern.  false: fewer than k points within max_ring cells.
__device__ __forceinline__ bool knn_radius(const KnnGrid& g, const float q[3], const int c[3], int k, int max_ring, int& R, float& r2) {
    float rmax2 = 0.f;
    bool ok = false;
    for (R = 1; R <= max_ring; ++R) {
        const float rr = (float)R * g.cell;          // the ball of radius R*cell around q lies inside the (2R+1)^3 block around q's cell
        rmax2 = rr * rr;
        if (count_within(g, q, c, R, rmax2) >= k) { ok = true; break; }
    }
    if (!ok) return false;
    unsigned lo = 0u, hi = __float_as_uint(rmax2);   // count(lo) may be < k, count(hi) >= k
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (count_within(g, q, c, R, __uint_as_float(mid)) >= k) hi = mid; else lo = mid + 1;
    }
    r2 = __uint_as_float(lo);
    return true;
}

// The neighbour set of radius r2: every candidate closer than r2 plus, of the ones AT r2, as many as still fit (walk order) --
// exactly k, like a kd-tree search (ties have measure zero on real data).  f as in knn_block.
template <typename F>
__device__ __forceinline__ void knn_visit(const KnnGrid& g, const float q[3], const int c[3], int R, float r2, int k, F f) {
    int ties_left = k;
    knn_block(g, q, c, R, [&](int, float, float, float, float d2) { ties_left -= d2 < r2; });
    knn_block(g, q, c, R, [&](int kk, float ex, float ey, float ez, float d2) {
        const bool tie = d2 == r2 && ties_left > 0;
        ties_left -= tie;
        if (d2 < r2 || tie) f(kk, ex, ey, ez, d2);
    });
}
