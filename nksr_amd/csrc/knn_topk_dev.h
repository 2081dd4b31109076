// Neighbour search over a Morton-sorted cloud, k <= 32 (nksr_amd/neighbours.py: PointGrid, PointPyramid).  What is in this file:
//
//   3. k <= 32: the register-list search.  TopK (the k nearest candidates sorted in registers), knn_scan, knn_rings (one grid scale,
//      cells nearest first, box pruning).
//   4. The octree: KnnPyramid, knn_descend, knn_topk_pyramid (every scale in one launch; a single grid is the octree with one level),
//      the exhaustive knn_topk_all behind the mesh metrics, and the host side every pyramid entry point shares (make_pyramid,
//      KNN_PYR_DISPATCH).
// Used by knn_sdf.hip (k_sdf_pyramid, k_knn_mean_dist_pyramid), knn_query.hip (k_knn_query_pyramid) and metrics.hip (k_nn_metrics).
// Queries run in Morton order where they are the cloud itself: neighbouring lanes scan the same cells.
#pragma once
#include "common.h"
#include "knn_dev.h"

// (The bisection and the two operations the next comment speaks of: knn_walk_dev.h, and k_sdf_from_points / k_knn_mean_dist in knn_sdf.hip.)
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
// candidates [s, e) of the sorted cloud into the list (knn_scan4: four at a time)
template <int KMAX>
__device__ __forceinline__ void knn_scan(const float* __restrict__ xyz, int s, int e, const float q[3], TopK<KMAX>& top) {
    knn_scan4(xyz, s, e, q, [&](int kk, float d2) { top.insert(d2, kk); });
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

// Every query gets its k nearest, whatever the pyramid search can reach: the box-pruned pass over ALL top-level cells -- the cell of
// the nearest box first, then every cell whose box is not farther than the best candidate so far, each descended like any other.
// The top level has a handful of cells (PointPyramid stops at <= 8).  (k_nn_metrics, metrics.hip: a query farther from the cloud than
// max_ring rings of the top level, or with a cell index outside the biased 21-bit key range.)
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

// ---- host side ------------------------------------------------------------------------------------------------------------------------
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
