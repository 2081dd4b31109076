// Neighbour search over a Morton-sorted cloud (nksr_amd/neighbours.py: PointGrid = the sorted points, the point range of every
// occupied cell and the cell hash; PointPyramid = an octree of such levels over the same points).  What is in this file:
//
//   1. One grid, any k: the block walk and the bisection.
//        knn_block        the cells c + [-R, R]^3 in a fixed order, every candidate handed to a visitor with knn_d2 of its offset
//        knn_radius       smallest ring whose inscribed ball holds k points, then the EXACT k-th smallest squared distance by a 32-step
//                         bisection on the float bit pattern (positive floats order like their bit patterns), each step re-counting
//                         the block (L1/L2 resident): exact selection without a per-thread heap
//        knn_visit        the k neighbours that radius defines, in walk order
//      k_knn_pca_normals  nksr_knn_pca_normals (nksr_amd/normals.py, kNN-PCA normals: nksr.get_estimate_normal_preprocess_fn, CPU
//                         recipe examples/recons_waymo_cpu.py:21-41): one thread per query -- every query when k > KW_CAP or no work
//                         array is given, else the queries k_knn_pca_wave hands back.  fp32 distances decide everything except the
//                         few candidates within a couple of ulps of the k-th distance: those are ranked by their fp64 distance, so
//                         the neighbour SET is the one an fp64 kd-tree search returns (an fp32-only rule swaps near-equidistant
//                         neighbours against it: normals off by ~1e-3 at a few points); mean and covariance in fp64 over that set.
//                         (The normals keep the bisection: their queries ARE the cloud -- always near -- and the fp64 tie rule needs
//                         the candidates AT the k-th distance, which a fixed-size list does not hold.)
//      k_knn_pca_wave     the same, one wavefront per query over an LDS candidate list (the default of nksr_knn_pca_normals)
//      k_nearest_index    nksr_nearest_index (PointGrid.nearest: the colour lookup of fields.PCNNField)
//      k_sdf_from_points, k_knn_mean_dist      nksr_sdf_from_points, nksr_knn_mean_dist (ext.sdfgen with nb_points > 32, on plain grids)
//   2. The two estimators of ext.sdfgen.sdf_from_points (SdfVote, SdfImls; reference ext/sdfgen/sdf_from_points.cu:32-140, call sites
//      models/loss.py:85, dataset/av_gt_geometry.py:72), each stated once and fed by both searches.
//   3. k <= 32: the register-list search.  TopK (the k nearest candidates sorted in registers), knn_scan, knn_rings (one grid scale,
//      cells nearest first, box pruning).
//   4. The octree: KnnPyramid, knn_descend, knn_topk_pyramid (every scale in one launch; a single grid is the octree with one level),
//      k_pyramid_level (nksr_knn_pyramid_level builds a level), and on them k_sdf_pyramid (nksr_sdf_from_points_pyramid),
//      k_knn_mean_dist_pyramid (nksr_knn_mean_dist_pyramid: the adaptive_knn radius of ext.sdfgen).
//   5. Metric and query kernels: k_nn_metrics (nksr_nn_metrics, nksr_amd/metrics.py: exact 1-NN with the mesh-metric epilogue, the
//      exhaustive knn_topk_all behind it), k_knn_query_pyramid (nksr_knn_query_pyramid, nksr_amd/cloud.py and orient.py: the k
//      nearest written out), k_radius_count (nksr_radius_count: the 27 cells of a grid with cell >= radius).
// Queries run in Morton order where they are the cloud itself: neighbouring lanes scan the same cells.
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

// smallest eigenvector of a symmetric 3x3 matrix (cyclic Jacobi, fp64)
__device__ void smallest_eigvec(double a[3][3], float nrm[3]) {
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off < 1e-30) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(a[p][q]) < 1e-300) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = cs * akp - sn * akq;
                    a[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = cs * apk - sn * aqk;
                    a[q][k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
    int m = 0;
    if (a[1][1] < a[m][m]) m = 1;
    if (a[2][2] < a[m][m]) m = 2;
    nrm[0] = (float)v[0][m];
    nrm[1] = (float)v[1][m];
    nrm[2] = (float)v[2][m];
}

__global__ void __launch_bounds__(128) k_knn_pca_normals(KnnGrid g, int64_t n, int k, int max_ring,
                                                         float* __restrict__ normal, float* __restrict__ radius2,
                                                         int32_t* __restrict__ valid, const int32_t* __restrict__ todo) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (todo && !todo[i]) return;          // (fallback pass: only the queries the wave-per-query kernel handed back)
    const float q[3] = {g.xyz[i * 3], g.xyz[i * 3 + 1], g.xyz[i * 3 + 2]};
    int c[3], R;
    float r2;
    cell_of(g, q, c);
    if (!knn_radius(g, q, c, k, max_ring, R, r2)) {   // fewer than k points within max_ring cells: isolated point
        valid[i] = 0;
        normal[i * 3] = normal[i * 3 + 1] = 0.f;
        normal[i * 3 + 2] = 1.f;
        radius2[i] = 0.f;
        return;
    }
    // candidates with an fp32 distance well below r2 are neighbours; the ones within a few ulps of it are ranked in fp64
    const float r2_lo = r2 * (1.0f - 2e-6f), r2_hi = r2 * (1.0f + 2e-6f);
    auto dist64 = [&](int kk) {
        const double fx = (double)g.xyz[kk * 3] - (double)q[0], fy = (double)g.xyz[kk * 3 + 1] - (double)q[1],
                     fz = (double)g.xyz[kk * 3 + 2] - (double)q[2];
        return fx * fx + fy * fy + fz * fz;
    };
    constexpr int AMB = 12;
    double amb[AMB];
    int n_amb = 0, n_in = 0;
    knn_block(g, q, c, R, [&](int kk, float, float, float, float d32) {
        if (d32 < r2_lo) { ++n_in; return; }
        if (d32 > r2_hi) return;
        const double d64 = dist64(kk);
        if (n_amb < AMB || d64 < amb[AMB - 1]) {          // insertion into the (tiny) ascending list: a full one drops its last
            int j = n_amb < AMB ? n_amb++ : AMB - 1;
            while (j > 0 && amb[j - 1] > d64) { amb[j] = amb[j - 1]; --j; }
            amb[j] = d64;
        }
    });
    int need = k - n_in;                         // how many of the near-threshold candidates belong to the k nearest
    if (need > n_amb) need = n_amb;
    const double thr64 = need > 0 ? amb[need - 1] : -1.0;
    // mean and covariance of the neighbour set
    double m[3] = {0, 0, 0};
    int cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
        double cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        knn_block(g, q, c, R, [&](int kk, float, float, float, float d32) {
            if (d32 > r2_hi || (d32 >= r2_lo && dist64(kk) > thr64)) return;
            const float px = g.xyz[kk * 3], py = g.xyz[kk * 3 + 1], pz = g.xyz[kk * 3 + 2];
            if (pass == 0) { m[0] += px; m[1] += py; m[2] += pz; ++cnt; }
            else {
                const double d0 = px - m[0], d1 = py - m[1], d2 = pz - m[2];
                cov[0][0] += d0 * d0; cov[0][1] += d0 * d1; cov[0][2] += d0 * d2;
                cov[1][1] += d1 * d1; cov[1][2] += d1 * d2; cov[2][2] += d2 * d2;
            }
        });
        if (pass == 0) { m[0] /= cnt; m[1] /= cnt; m[2] /= cnt; }
        else {
            cov[1][0] = cov[0][1]; cov[2][0] = cov[0][2]; cov[2][1] = cov[1][2];
            float nv[3];
            smallest_eigvec(cov, nv);
            normal[i * 3] = nv[0]; normal[i * 3 + 1] = nv[1]; normal[i * 3 + 2] = nv[2];
        }
    }
    radius2[i] = r2;
    valid[i] = 1;
}

// ---- one WAVEFRONT per query (the default) -------------------------------------------------------------------------------------
// The thread-per-query kernel above walks ~36 times over the ~400 candidates of its block, one dependent load after the other:
// fine when a million queries hide each other's latency, 52 ms for the 10 000-point scan of examples/recons_waymo_cpu.py (40
// wavefronts on 256 CUs).  Here the 64 lanes of a wavefront share one query: the candidates of the (2R+1)^3 block are gathered ONCE
// into LDS as (squared distance, point index) -- lane = cell of the block, offsets from a wave prefix sum over the cells' point
// counts, so the candidate order is the cell order: deterministic -- and every later pass (ring count, the 32-step bit-pattern
// bisection, the fp64 ranking of the candidates within a few ulps of the k-th distance, mean, covariance) strides over that list
// with ballot / fixed-tree reductions.  Same selection rule, same r2, same neighbour SET as the thread-per-query kernel (which
// stays as the fallback for a query whose block holds more than KW_CAP candidates: `todo`).
#define KW_CAP 2048
#define KW_WAVES 4
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(64 * KW_WAVES) k_knn_pca_wave(KnnGrid g, int64_t n, int k, int max_ring, float* __restrict__ normal,
                                                               float* __restrict__ radius2, int32_t* __restrict__ valid,
                                                               int32_t* __restrict__ todo) {
    __shared__ float cd[KW_WAVES][KW_CAP];
    __shared__ int32_t ci[KW_WAVES][KW_CAP];
    __shared__ double amb[KW_WAVES][16];
    // 64.5 KB of static LDS per workgroup: written for the 160 KB per CU of gfx950 (two workgroups = eight wavefronts per CU); a
    // 64 KB-LDS part (gfx942 / gfx90a) would need KW_WAVES 2
    static_assert(sizeof(float) * KW_WAVES * KW_CAP + sizeof(int32_t) * KW_WAVES * KW_CAP + sizeof(double) * KW_WAVES * 16 <= 80 * 1024,
                  "k_knn_pca_wave: two workgroups must fit the 160 KB LDS of a gfx950 CU");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * KW_WAVES + wave;
    if (i >= n) return;
    float* d2 = cd[wave];
    int32_t* idx = ci[wave];
    const float q[3] = {g.xyz[i * 3], g.xyz[i * 3 + 1], g.xyz[i * 3 + 2]};
    int c[3];
    cell_of(g, q, c);
    int ncand = 0, R = 1;
    float rmax2 = 0.f;
    bool ok = false, overflow = false;
    for (; R <= max_ring; ++R) {
        const int side = 2 * R + 1, ncell = side * side * side;
        ncand = 0;
        for (int base = 0; base < ncell && !overflow; base += 64) {
            const int cc = base + lane;
            int s0 = 0, s1 = 0;
            if (cc < ncell) {
                const int dx = cc / (side * side) - R, dy = (cc / side) % side - R, dz = cc % side - R;
                const int cell = hash_find(g.hkeys, g.hvals, g.hcap, morton_biased(c[0] + dx, c[1] + dy, c[2] + dz, NKSR_BIAS0));
                if (cell >= 0) { s0 = g.start[cell]; s1 = g.end[cell]; }
            }
            int cnt = s1 - s0, off = cnt;                          // inclusive prefix sum over the lanes (= the cells, in block order)
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(off, o);
                if (lane >= o) off += t;
            }
            const int total = __shfl(off, 63);
            if (ncand + total > KW_CAP) { overflow = true; break; }
            int w = ncand + off - cnt;
            for (int p = s0; p < s1; ++p, ++w) {
                const float ex = g.xyz[(int64_t)p * 3] - q[0], ey = g.xyz[(int64_t)p * 3 + 1] - q[1], ez = g.xyz[(int64_t)p * 3 + 2] - q[2];
                d2[w] = knn_d2(ex, ey, ez);
                idx[w] = p;
            }
            ncand += total;
        }
        if (overflow) break;
        __builtin_amdgcn_wave_barrier();
        const float rr = (float)R * g.cell;
        rmax2 = rr * rr;
        int cnt = 0;
        for (int j = lane; j - lane < ncand; j += 64) cnt += __popcll(__ballot(j < ncand && d2[j] <= rmax2));
        if (cnt >= k) { ok = true; break; }
    }
    if (overflow) {                 // too many candidates for the LDS list: the thread-per-query kernel takes this query
        if (lane == 0) todo[i] = 1;
        return;
    }
    if (lane == 0) todo[i] = 0;
    if (!ok) {   // fewer than k points within max_ring cells: isolated point
        if (lane == 0) {
            valid[i] = 0;
            normal[i * 3] = normal[i * 3 + 1] = 0.f;
            normal[i * 3 + 2] = 1.f;
            radius2[i] = 0.f;
        }
        return;
    }
    // exact k-th smallest squared distance: bisection on the bit pattern
    unsigned lo = 0u, hi = __float_as_uint(rmax2);
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        const float m = __uint_as_float(mid);
        int cnt = 0;
        for (int j = lane; j - lane < ncand; j += 64) cnt += __popcll(__ballot(j < ncand && d2[j] <= m));
        if (cnt >= k) hi = mid; else lo = mid + 1;
    }
    const float r2 = __uint_as_float(lo);
    // candidates with an fp32 distance well below r2 are neighbours; the ones within a few ulps of it are ranked in fp64
    const float r2_lo = r2 * (1.0f - 2e-6f), r2_hi = r2 * (1.0f + 2e-6f);
    int n_in = 0, n_amb = 0;
    for (int j = lane; j - lane < ncand; j += 64) {
        const bool in = j < ncand;
        const float d = in ? d2[j] : 3.4e38f;
        n_in += __popcll(__ballot(in && d < r2_lo));
        const bool am = in && d >= r2_lo && d <= r2_hi;
        const unsigned long long mask = __ballot(am);
        if (am) {
            const int slot = n_amb + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < 16) {
                const int p = idx[j];
                const double fx = (double)g.xyz[(int64_t)p * 3] - (double)q[0], fy = (double)g.xyz[(int64_t)p * 3 + 1] - (double)q[1],
                             fz = (double)g.xyz[(int64_t)p * 3 + 2] - (double)q[2];
                amb[wave][slot] = fx * fx + fy * fy + fz * fz;
            }
        }
        n_amb += __popcll(mask);
    }
    __builtin_amdgcn_wave_barrier();
    if (n_amb > 16) n_amb = 16;                  // (more than 16 candidates within 2e-6 of the k-th distance: degenerate input)
    int need = k - n_in;
    if (need > n_amb) need = n_amb;
    double thr64 = -1.0;
    if (need > 0) {                              // the need-th smallest of <= 16 values: every lane ranks them (uniform result)
        double best = -1.0;
        for (int a = 0; a < n_amb; ++a) {
            const double v = amb[wave][a];
            int rank = 0;
            for (int b = 0; b < n_amb; ++b) rank += (amb[wave][b] < v) || (amb[wave][b] == v && b < a);
            if (rank == need - 1) best = v;
        }
        thr64 = best;
    }
    // mean and covariance of the neighbour set (fp64, lane-strided partial sums + a fixed reduction tree)
    double m[3] = {0, 0, 0};
    int cntn = 0;
    for (int pass = 0; pass < 2; ++pass) {
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0;
        int cl = 0;
        for (int j = lane; j < ncand; j += 64) {
            const float d = d2[j];
            if (d > r2_hi) continue;
            const int p = idx[j];
            const float px = g.xyz[(int64_t)p * 3], py = g.xyz[(int64_t)p * 3 + 1], pz = g.xyz[(int64_t)p * 3 + 2];
            if (d >= r2_lo) {
                const double fx = (double)px - (double)q[0], fy = (double)py - (double)q[1], fz = (double)pz - (double)q[2];
                if (fx * fx + fy * fy + fz * fz > thr64) continue;
            }
            if (pass == 0) { a0 += px; a1 += py; a2 += pz; ++cl; }
            else {
                const double e0 = px - m[0], e1 = py - m[1], e2 = pz - m[2];
                a0 += e0 * e0; a1 += e0 * e1; a2 += e0 * e2; a3 += e1 * e1; a4 += e1 * e2; a5 += e2 * e2;
            }
        }
        a0 = wave_sum_d(a0); a1 = wave_sum_d(a1); a2 = wave_sum_d(a2);
        if (pass == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cl += __shfl_xor(cl, o);
            cntn = cl;
            m[0] = a0 / cntn; m[1] = a1 / cntn; m[2] = a2 / cntn;
        } else {
            a3 = wave_sum_d(a3); a4 = wave_sum_d(a4); a5 = wave_sum_d(a5);
            if (lane == 0) {
                double cov[3][3] = {{a0, a1, a2}, {a1, a3, a4}, {a2, a4, a5}};
                float nv[3];
                smallest_eigvec(cov, nv);
                normal[i * 3] = nv[0]; normal[i * 3 + 1] = nv[1]; normal[i * 3 + 2] = nv[2];
                radius2[i] = r2;
                valid[i] = 1;
            }
        }
    }
}

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

// ---- the same two operations with ONE scan per ring: the k nearest candidates kept in registers -------------------------------------
// The bisection above scans the candidate block ~35 times per query (ring search + 32 bit-steps + the visits).  For k <= 32 a
// thread keeps the k smallest (distance, index) pairs sorted in registers and inserts every candidate once (an unrolled
// compare-and-shift over KMAX slots; a candidate AT the k-th distance does not displace one seen earlier), ring after ring
// (only the new shell of cells is scanned) until the k-th distance lies inside the scanned block.  Measured against the
// REFERENCE'S OWN extension on the same MI355X (tests/sdfgen_vs_ref.py, profiles/r04_sdfgen_vs_reference.md): with the bisection
// 44 ms against the reference's 3.0 ms at 4 000 reference points / 1 000 queries and 2.7 s against 20 ms at 1 M / 1 M; with
// everything below 1.0 ms and 13.8 ms.
template <int KMAX>
struct TopK {
    // The k candidates live in the LAST k slots (ascending); the KMAX - k slots before them hold a sentinel below every distance and
    // are never displaced.  The k-th candidate is therefore always slot KMAX - 1, a fixed register: indexed by k it was a select
    // chain that the compiler turned into an indexed load from a scratch copy of the arrays, written back after every scanned cell.
    float d2[KMAX];
    int idx[KMAX];
    bool any;
    __device__ __forceinline__ void init(int k) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { d2[j] = j < KMAX - k ? -1.f : 3.4e38f; idx[j] = -1; }
        any = false;
    }
    __device__ __forceinline__ void insert(float d, int id) {
        if (!(d < d2[KMAX - 1])) return;
        any = true;
#pragma unroll
        for (int j = KMAX - 1; j >= 1; --j) {
            const bool shift = d < d2[j - 1];
            const bool here = !shift && d < d2[j];
            d2[j] = shift ? d2[j - 1] : (here ? d : d2[j]);
            idx[j] = shift ? idx[j - 1] : (here ? id : idx[j]);
        }
        if (d < d2[0]) { d2[0] = d; idx[0] = id; }
    }
    __device__ __forceinline__ float kth() const { return d2[KMAX - 1]; }               // 3.4e38 while fewer than k were seen
    __device__ __forceinline__ bool full() const { return d2[KMAX - 1] < 3.4e38f; }
};
// candidates [s, e) of the sorted cloud, four at a time: the twelve coordinate loads of a group are in flight together (one at a time,
// a cell of 30 points was 30 memory latencies end to end -- the insertion needs each distance before the next)
template <int KMAX>
__device__ __forceinline__ void knn_scan(const float* __restrict__ xyz, int s, int e, const float q[3], TopK<KMAX>& top) {
    int kk = s;
    for (; kk + 4 <= e; kk += 4) {
        float p[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) p[t] = xyz[kk * 3 + t];
#pragma unroll
        for (int t = 0; t < 4; ++t) top.insert(knn_d2(p[3 * t] - q[0], p[3 * t + 1] - q[1], p[3 * t + 2] - q[2]), kk + t);
    }
    for (; kk < e; ++kk) top.insert(knn_d2(xyz[kk * 3] - q[0], xyz[kk * 3 + 1] - q[1], xyz[kk * 3 + 2] - q[2]), kk);
}
// The search itself, for ONE grid scale.  Cells are handed to `visit(cx, cy, cz)` in this order: the 27 cells around q's cell c
// NEAREST FIRST (by the distance of their box from q -- separable, one squared gap per axis and side; q's own cell has gap 0 and
// comes first), stopping at the first cell farther than the current k-th candidate: a query next to the surface looks at 3-5 cells
// instead of 27.  Then, only while the k-th candidate lies outside the scanned block, the shells R = 2 .. max_ring, every cell whose
// BOX is farther than the k-th candidate skipped without a look-up (the gap is shortened by 2 % of a cell against the fp32
// rounding of the box bounds c * cell at large coordinates).  Returns 1: the k nearest are in `top`; 0: fewer than k inside
// max_ring rings; -1: NOTHING within one cell (q is far from the cloud on this scale).
template <int KMAX, class Visit>
__device__ __forceinline__ int knn_rings(float cellsz, const float q[3], const int c[3], int k, int max_ring, bool coarser_exists,
                                         TopK<KMAX>& top, Visit&& visit) {
    top.init(k);
    const float slack = 0.02f * cellsz;
    float gs[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = (float)c[a] * cellsz;
        const float em = fmaxf(q[a] - lo - slack, 0.f), ep = fmaxf(lo + cellsz - q[a] - slack, 0.f);
        gs[a][0] = em * em; gs[a][1] = 0.f; gs[a][2] = ep * ep;
    }
    unsigned visited = 0u;
    int R = 1, dx = 0, dy = 0, dz = 0;
    for (;;) {
        int ox, oy, oz;
        if (R == 1) {
            float best = 3.4e38f;
            int bi = -1;
#pragma unroll
            for (int j = 0; j < 27; ++j) {
                const float gj = gs[0][j / 9] + gs[1][(j / 3) % 3] + gs[2][j % 3];
                if (!((visited >> j) & 1u) && gj < best) { best = gj; bi = j; }
            }
            if (bi < 0 || best > top.kth()) {
                if (top.kth() <= cellsz * cellsz) return 1;
                if (!top.any) return -1;
                // fewer than k candidates so far: nothing prunes the wider shells (98, 218, 386 look-ups) -- a coarser scale, if there
                // is one, reaches the same points in 27
                if (max_ring < 2 || (coarser_exists && !top.full())) return 0;
                R = 2; dx = dy = dz = -2;
                continue;
            }
            visited |= 1u << bi;
            ox = bi / 9 - 1; oy = (bi / 3) % 3 - 1; oz = bi % 3 - 1;
        } else {
            if (dx > R) {                                   // shell R done: the ball of radius R * cell around q lies inside the block
                const float rr = (float)R * cellsz;
                if (top.kth() <= rr * rr) return 1;
                if (++R > max_ring || (coarser_exists && !top.full())) return 0;
                dx = dy = dz = -R;
                continue;
            }
            ox = dx; oy = dy; oz = dz;
            const bool inner = abs(dx) < R && abs(dy) < R;  // (inside the shell only its two z faces are new)
            dz += inner ? 2 * R : 1;
            if (dz > R) { dz = -R; if (++dy > R) { dy = -R; ++dx; } }
            float gap2 = 0.f;
            const int cc[3] = {c[0] + ox, c[1] + oy, c[2] + oz};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float lo = (float)cc[a] * cellsz, hi = lo + cellsz;
                const float e = fmaxf(fmaxf(lo - q[a], q[a] - hi) - slack, 0.f);
                gap2 = fmaf(e, e, gap2);
            }
            if (gap2 > top.kth()) continue;
        }
        visit(c[0] + ox, c[1] + oy, c[2] + oz);
    }
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

// ---- every scale in one launch: an octree over the same Morton-sorted points ---------------------------------------------------------
// Level l has cells of size cell * 2^l; its cell keys are the level-0 keys >> 3 l, so a level-l cell is a contiguous range of the
// sorted points AND of the level-(l-1) cells (its <= 8 children, in octant order: child[l][i] .. child[l][i + 1], cmask[l][i] = the
// occupied octants).  A query climbs to the first level with anything within one cell of it (27 look-ups per level -- a far query
// leaves the fine levels at once), and searches THAT scale with knn_rings; a cell there is not scanned but DESCENDED: children
// nearest octant first, every child whose box lies farther than the current k-th candidate cut off, points scanned only in
// cells of <= leaf points.  A query at distance d from the cloud therefore costs ~log(d / cell) box tests plus the few leaves that
// face it -- on the single coarse grid of the host's round loop (x4 cell per round, 16x points per cell) it scanned whole cells
// of thousands of points, 14 ms for the last 16 000 queries of 1 M.  The descent keeps one (node, cursor) pair per level in LDS --
// and so does the table of per-level pointers: indexed by a per-lane level IN THE KERNEL ARGUMENTS it was a vector load from the
// kernarg segment (host-visible, uncached) at every step, 1.7 ms for 4 000 queries that now take a fraction of it.
struct KnnPyramid {
    const int32_t* start[NKSR_KNN_LEVELS];
    const int32_t* end[NKSR_KNN_LEVELS];
    const int32_t* child[NKSR_KNN_LEVELS];
    const uint8_t* cmask[NKSR_KNN_LEVELS];
    const int64_t* hkeys[NKSR_KNN_LEVELS];
    const int32_t* hvals[NKSR_KNN_LEVELS];
    int hcap[NKSR_KNN_LEVELS];
    int levels, leaf;
    const float* xyz;
    float cell, inv_cell;
};
#define KNN_PYR_BLOCK 128
// cell ci = (cx, cy, cz) of level l: scanned when it is a leaf, else descended (children nearest octant first, every child whose box
// lies farther than the current k-th candidate cut off) down to leaves of <= P.leaf points
template <int KMAX>
__device__ __forceinline__ void knn_descend(const KnnPyramid& P, int l, int ci, int cx, int cy, int cz, const float q[3], TopK<KMAX>& top,
                                            int* node, unsigned char* cursor) {
    int lvl = l;
    bool enter = true;
    for (;;) {
        if (enter) {
            const int s = P.start[lvl][ci], e = P.end[lvl][ci];
            if (lvl == 0 || e - s <= P.leaf) {
                knn_scan<KMAX>(P.xyz, s, e, q, top);
                if (lvl == l) return;
                ++lvl; cx >>= 1; cy >>= 1; cz >>= 1;               // back to the parent
            } else {
                node[lvl * KNN_PYR_BLOCK] = ci;
                cursor[lvl * KNN_PYR_BLOCK] = 0;
            }
            enter = false;
            continue;
        }
        // the next child of node[lvl] (cell (cx, cy, cz) of level lvl) worth a visit
        const int nd = node[lvl * KNN_PYR_BLOCK];
        int t = cursor[lvl * KNN_PYR_BLOCK];
        const unsigned mask = P.cmask[lvl][nd];
        const float cl = P.cell * (float)(1 << lvl), ch = 0.5f * cl, slack = 0.02f * ch;
        const unsigned qo = (q[0] >= ((float)cx + 0.5f) * cl ? 1u : 0u) | (q[1] >= ((float)cy + 0.5f) * cl ? 2u : 0u) |
                            (q[2] >= ((float)cz + 0.5f) * cl ? 4u : 0u);
        bool found = false;
        while (t < 8) {
            const unsigned o = ((0x76534210u >> (4 * t)) & 7u) ^ qo;      // octants by the number of axes they differ from q's in
            ++t;
            if (!((mask >> o) & 1u)) continue;
            const int x = 2 * cx + (int)(o & 1u), y = 2 * cy + (int)((o >> 1) & 1u), z = 2 * cz + (int)(o >> 2);
            const float lo[3] = {(float)x * ch, (float)y * ch, (float)z * ch};
            float gap2 = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float e = fmaxf(fmaxf(lo[a] - q[a], q[a] - (lo[a] + ch)) - slack, 0.f);
                gap2 = fmaf(e, e, gap2);
            }
            if (gap2 > top.kth()) continue;
            ci = P.child[lvl][nd] + __popc(mask & ((1u << o) - 1u));
            cx = x; cy = y; cz = z;
            found = true;
            break;
        }
        if (found) {
            cursor[lvl * KNN_PYR_BLOCK] = (unsigned char)t;
            --lvl;
            enter = true;
        } else {
            if (lvl == l) return;
            ++lvl; cx >>= 1; cy >>= 1; cz >>= 1;
        }
    }
}
template <int KMAX>
__device__ __forceinline__ bool knn_topk_pyramid(const KnnPyramid& P, const float q[3], int k, int max_ring, TopK<KMAX>& top, int* node,
                                                 unsigned char* cursor) {
    int c0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float p;
        c0[a] = half_index(q[a], P.inv_cell, p) >> 1;
    }
    // the finest level with anything in the 27 cells around q: "occupied" is monotone in the level (the block of level l + 1 covers
    // the block of level l), so after level 0 it is bisected -- a far query pays ~4 probes, most of them ended by an early hit
    auto occupied = [&](int l) {
        const int bias = NKSR_BIAS0 >> l;
        for (int j = 0; j < 27; ++j)
            if (hash_find(P.hkeys[l], P.hvals[l], P.hcap[l],
                          morton_biased((c0[0] >> l) + j / 9 - 1, (c0[1] >> l) + (j / 3) % 3 - 1, (c0[2] >> l) + j % 3 - 1, bias)) >= 0)
                return true;
        return false;
    };
    int first = 0;
    if (P.levels > 1 && !occupied(0)) {
        int lo = 0;
        first = P.levels - 1;
        while (first - lo > 1) {
            const int mid = (lo + first) >> 1;
            if (occupied(mid)) first = mid; else lo = mid;
        }
    }
    for (int l = first; l < P.levels; ++l) {
        const float cell_l = P.cell * (float)(1 << l);
        const int c[3] = {c0[0] >> l, c0[1] >> l, c0[2] >> l};
        const int rc = knn_rings<KMAX>(cell_l, q, c, k, max_ring, l + 1 < P.levels, top, [&](int cx, int cy, int cz) {
            const int ci = hash_find(P.hkeys[l], P.hvals[l], P.hcap[l], morton_biased(cx, cy, cz, NKSR_BIAS0 >> l));
            if (ci < 0) return;
            knn_descend<KMAX>(P, l, ci, cx, cy, cz, q, top, node, cursor);
        });
        if (rc == 1) return true;
    }
    return false;
}
// How every pyramid kernel starts: the pyramid copied from the kernel arguments into LDS (by thread 0, then a barrier: EVERY thread of the
// workgroup must come here), and this thread's column of the descent stacks, one (node, cursor) pair per level.  Three separate LDS
// arrays, as they were when each kernel declared its own: packed into one struct the kernels came out with other register counts.
__device__ __forceinline__ const KnnPyramid& knn_pyramid_lds(const KnnPyramid& Parg, int*& node, unsigned char*& cursor) {
    __shared__ int s_node[NKSR_KNN_LEVELS][KNN_PYR_BLOCK];
    __shared__ unsigned char s_cursor[NKSR_KNN_LEVELS][KNN_PYR_BLOCK];
    __shared__ KnnPyramid P;
    if (threadIdx.x == 0) P = Parg;
    __syncthreads();
    node = &s_node[0][threadIdx.x];
    cursor = &s_cursor[0][threadIdx.x];
    return P;
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

extern "C" int nksr_knn_pca_normals(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end,
                                    const int64_t* hkeys, const int32_t* hvals, int32_t hcap, float cell, float inv_cell, int k, int max_ring,
                                    float* normal_out, float* radius2_out, int32_t* valid_out, int32_t* todo_work, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (k < 3) return nksr_set_error(NKSR_ERR_ARG, "knn must be >= 3");
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    if (!todo_work || k > KW_CAP) {        // no work array: thread-per-query for all
        hipLaunchKernelGGL(k_knn_pca_normals, dim3(nksr_blocks(n, 128)), dim3(128), 0, (hipStream_t)stream, g, n, k, max_ring,
                           normal_out, radius2_out, valid_out, (const int32_t*)nullptr);
    } else {
        hipLaunchKernelGGL(k_knn_pca_wave, dim3(nksr_blocks(n, KW_WAVES)), dim3(64 * KW_WAVES), 0, (hipStream_t)stream, g, n, k, max_ring,
                           normal_out, radius2_out, valid_out, todo_work);
        hipLaunchKernelGGL(k_knn_pca_normals, dim3(nksr_blocks(n, 128)), dim3(128), 0, (hipStream_t)stream, g, n, k, max_ring,
                           normal_out, radius2_out, valid_out, (const int32_t*)todo_work);
    }
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
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

// The pyramid kernels are templates over the size of the register list: KERNEL<8 / 16 / 32 / KLAST> for `slots` <= 8 / 16 / 32 / more
// (KLAST = 32 where the entry point admits no more than 32), one thread per row, on `stream` of the calling function.
#define KNN_PYR_LAUNCH(KERNEL, KM, rows, ...) \
    hipLaunchKernelGGL((KERNEL<KM>), dim3(nksr_blocks(rows, KNN_PYR_BLOCK)), dim3(KNN_PYR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__)
#define KNN_PYR_DISPATCH(KERNEL, KLAST, slots, rows, ...)                  \
    do {                                                                   \
        if ((slots) <= 8) KNN_PYR_LAUNCH(KERNEL, 8, rows, __VA_ARGS__);    \
        else if ((slots) <= 16) KNN_PYR_LAUNCH(KERNEL, 16, rows, __VA_ARGS__); \
        else if ((slots) <= 32) KNN_PYR_LAUNCH(KERNEL, 32, rows, __VA_ARGS__); \
        else KNN_PYR_LAUNCH(KERNEL, KLAST, rows, __VA_ARGS__);             \
    } while (0)
static int make_pyramid(KnnPyramid& P, const nksr_knn_pyramid_t* p) {
    if (!p || p->levels < 1 || p->levels > NKSR_KNN_LEVELS || !p->xyz_sorted) return nksr_set_error(NKSR_ERR_ARG, "kNN pyramid: 1..%d levels", NKSR_KNN_LEVELS);
    memset(&P, 0, sizeof(P));
    for (int l = 0; l < p->levels; ++l) {
        if (!p->start[l] || !p->end[l] || !p->hkeys[l] || !p->hvals[l] || p->hcap[l] < 8 || (l > 0 && (!p->child[l] || !p->cmask[l])))
            return nksr_set_error(NKSR_ERR_ARG, "kNN pyramid: level %d incomplete", l);
        P.start[l] = p->start[l]; P.end[l] = p->end[l]; P.child[l] = p->child[l]; P.cmask[l] = p->cmask[l];
        P.hkeys[l] = p->hkeys[l]; P.hvals[l] = p->hvals[l]; P.hcap[l] = p->hcap[l];
    }
    P.levels = p->levels; P.leaf = p->leaf > 0 ? p->leaf : 48; P.xyz = p->xyz_sorted; P.cell = p->cell; P.inv_cell = p->inv_cell;
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

// ---- exact 1-NN of every query with the mesh-metric epilogue (nksr_amd/metrics.py) ----------------------------------------------------
// Every query gets its nearest point.  The pyramid search (k = 1) answers the queries it can reach; a query it cannot -- farther from
// the cloud than max_ring rings of the top level, or with a cell index outside the biased 21-bit key range -- takes the box-pruned pass
// over ALL top-level cells instead: the cell of the nearest box first, then every cell whose box is not farther than the best
// candidate so far, each descended like any other.  The top level has a handful of cells (PointPyramid stops at <= 8).
template <int KMAX>
__device__ __forceinline__ void knn_topk_all(const KnnPyramid& P, const int64_t* __restrict__ top_keys, int n_top, const float q[3], int k,
                                             TopK<KMAX>& top, int* node, unsigned char* cursor) {
    top.init(k);
    const int l = P.levels - 1;
    const float cl = P.cell * (float)(1 << l), slack = 0.02f * cl;
    auto gap = [&](int t, int c[3]) {
        morton_decode_biased(top_keys[t], NKSR_BIAS0 >> l, c[0], c[1], c[2]);
        float g2 = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = (float)c[a] * cl;
            const float e = fmaxf(fmaxf(lo - q[a], q[a] - (lo + cl)) - slack, 0.f);
            g2 = fmaf(e, e, g2);
        }
        return g2;
    };
    int best = -1, c[3];
    float bg = 3.4e38f;
    for (int t = 0; t < n_top; ++t) {
        const float g2 = gap(t, c);
        if (g2 < bg) { bg = g2; best = t; }
    }
    if (best < 0) return;
    gap(best, c);
    knn_descend<KMAX>(P, l, best, c[0], c[1], c[2], q, top, node, cursor);
    for (int t = 0; t < n_top; ++t) {
        if (t == best || gap(t, c) > top.kth()) continue;
        knn_descend<KMAX>(P, l, t, c[0], c[1], c[2], q, top, node, cursor);
    }
}
// One thread per query: dist = |q - p_nn| (fp64 from the fp32 coordinates), dot = |n_q . n_nn| of the two normals scaled to unit length
// (a zero normal gives 0).  Per workgroup, fp64 sums of d, d^2, dot and the counts of d <= t for the five thresholds, reduced over the
// block in a fixed tree order: the partials (and nksr_metric_reduce over them) are bitwise reproducible.
__global__ void __launch_bounds__(NKSR_NN_BLOCK) k_nn_metrics(KnnPyramid Parg, const int64_t* __restrict__ top_keys, int n_top,
                                                              const float* __restrict__ tnrm, const float* __restrict__ query,
                                                              const float* __restrict__ qnrm, int64_t nq, int max_ring, float* __restrict__ dist,
                                                              float* __restrict__ dot, double* __restrict__ partials) {
    static_assert(NKSR_NN_BLOCK == KNN_PYR_BLOCK, "one LDS slot row per thread");
    __shared__ double s_red[NKSR_METRIC_FIELDS][NKSR_NN_BLOCK];
    int* node;
    unsigned char* cursor;
    const KnnPyramid& P = knn_pyramid_lds(Parg, node, cursor);
    const int64_t i = (int64_t)blockIdx.x * NKSR_NN_BLOCK + threadIdx.x;
    double acc[NKSR_METRIC_FIELDS];
#pragma unroll
    for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) acc[f] = 0.0;
    if (i < nq) {
        const float q[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
        TopK<1> top;
        const float lim = (float)(NKSR_BIAS0 >> 1);           // cell indices well inside the biased key range
        const bool in_range = fabsf(q[0] * P.inv_cell) < lim && fabsf(q[1] * P.inv_cell) < lim && fabsf(q[2] * P.inv_cell) < lim;
        if (!in_range || !knn_topk_pyramid<1>(P, q, 1, max_ring, top, node, cursor))
            knn_topk_all<1>(P, top_keys, n_top, q, 1, top, node, cursor);
        const int j = top.idx[0];
        double d = __builtin_nan(""), dt = 0.0;
        if (j >= 0) {
            const double ex = (double)q[0] - (double)P.xyz[j * 3], ey = (double)q[1] - (double)P.xyz[j * 3 + 1],
                         ez = (double)q[2] - (double)P.xyz[j * 3 + 2];
            d = sqrt(ex * ex + ey * ey + ez * ez);
            if (tnrm && qnrm) {
                const double ax = qnrm[i * 3], ay = qnrm[i * 3 + 1], az = qnrm[i * 3 + 2];
                const double bx = tnrm[j * 3], by = tnrm[j * 3 + 1], bz = tnrm[j * 3 + 2];
                const double la = fmax(sqrt(ax * ax + ay * ay + az * az), 1e-30), lb = fmax(sqrt(bx * bx + by * by + bz * bz), 1e-30);
                dt = fabs(ax * bx + ay * by + az * bz) / (la * lb);
            }
        }
        if (dist) dist[i] = (float)d;
        if (dot) dot[i] = (float)dt;
        const double th[NKSR_METRIC_NTHRESH] = NKSR_METRIC_THRESHOLDS;
        acc[0] = d; acc[1] = d * d; acc[2] = dt;
#pragma unroll
        for (int t = 0; t < NKSR_METRIC_NTHRESH; ++t) acc[3 + t] = d <= th[t] ? 1.0 : 0.0;
    }
    if (!partials) return;
#pragma unroll
    for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) s_red[f][threadIdx.x] = acc[f];
    __syncthreads();
    for (int s = NKSR_NN_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) s_red[f][threadIdx.x] += s_red[f][threadIdx.x + s];
        __syncthreads();
    }
    if ((int)threadIdx.x < NKSR_METRIC_FIELDS) partials[(int64_t)blockIdx.x * NKSR_METRIC_FIELDS + threadIdx.x] = s_red[threadIdx.x][0];
}
extern "C" int nksr_nn_metrics(const nksr_knn_pyramid_t* pyramid, const int64_t* top_keys, int32_t n_top, const float* normal_sorted,
                               const float* query, const float* query_normal, int64_t nq, int max_ring, float* dist_out, float* dot_out,
                               double* partials_out, void* stream) {
    if (nq < 0 || n_top < 0) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: negative size (nq=%lld, n_top=%d)", (long long)nq, n_top);
    if (nq == 0) return NKSR_OK;
    if (!query || !top_keys || n_top < 1) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: NULL query / top-level keys or an empty target");
    if (!dist_out && !dot_out && !partials_out) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: no output (dist, dot and partials all NULL)");
    if (dot_out && (!normal_sorted || !query_normal)) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: dot output needs both normal arrays");
    if (max_ring < 1) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: max_ring must be >= 1 (got %d)", max_ring);
    KnnPyramid P;
    if (int rc = make_pyramid(P, pyramid)) return rc;
    hipLaunchKernelGGL(k_nn_metrics, dim3(nksr_blocks(nq, NKSR_NN_BLOCK)), dim3(NKSR_NN_BLOCK), 0, (hipStream_t)stream, P, top_keys, (int)n_top,
                       normal_sorted, query, query_normal, nq, max_ring, dist_out, dot_out, partials_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// ---- the k nearest WRITTEN OUT, and the points within a radius counted (nksr_amd/cloud.py) ---------------------------------------------
// The search is the one above (knn_topk_pyramid, one thread per query, the block shape and LDS stacks of k_sdf_pyramid);
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
// One thread per query, the 27 cells around it (cell >= radius: nothing within the radius lies outside them), candidates four at a time
// like knn_scan.  The count may pass `cap` by the rest of a group of four before the scan stops: clamped at the end.
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
    for (int j = 0; j < 27 && n < cap; ++j) {
        const int ci = hash_find(g.hkeys, g.hvals, g.hcap, morton_biased(c[0] + j / 9 - 1, c[1] + (j / 3) % 3 - 1, c[2] + j % 3 - 1, NKSR_BIAS0));
        if (ci < 0) continue;
        const int e = g.end[ci];
        int kk = g.start[ci];
        for (; kk + 4 <= e && n < cap; kk += 4) {
            float p[12];
#pragma unroll
            for (int t = 0; t < 12; ++t) p[t] = g.xyz[kk * 3 + t];
#pragma unroll
            for (int t = 0; t < 4; ++t) n += (kk + t != self) && knn_d2(p[3 * t] - q[0], p[3 * t + 1] - q[1], p[3 * t + 2] - q[2]) <= r2;
        }
        if (n >= cap) break;
        for (; kk < e; ++kk) n += (kk != self) && knn_d2(g.xyz[kk * 3] - q[0], g.xyz[kk * 3 + 1] - q[1], g.xyz[kk * 3 + 2] - q[2]) <= r2;
    }
    count[i] = n < cap ? n : cap;
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
    if (!(radius > 0.f) || !(radius < 3.4e38f)) return nksr_set_error(NKSR_ERR_ARG, "radius count: radius must be positive and finite");
    if (int rc = knn_grid_args("radius count", xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell)) return rc;
    if (!(cell >= radius)) return nksr_set_error(NKSR_ERR_ARG, "radius count: the grid's cell (%g) must be >= radius (%g)", (double)cell, (double)radius);
    if (!query && nq > n_ref) return nksr_set_error(NKSR_ERR_ARG, "radius count: query NULL (the cloud itself) with nq = %lld > n_ref = %lld", (long long)nq, (long long)n_ref);
    if (nq > 0 && !count_out) return nksr_set_error(NKSR_ERR_ARG, "radius count: NULL output array");
    if (nq == 0) return NKSR_OK;
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    hipLaunchKernelGGL(k_radius_count, dim3(nksr_blocks(nq, 128)), dim3(128), 0, (hipStream_t)stream, g, query, nq, radius * radius,
                       cap > 0 ? (int)cap : 0x7fffffff, exclude_self, self_index, count_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
