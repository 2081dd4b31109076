// The pass over the kernel rows of the matrix-free operator  y = (sum_s R_s^T R_s + reg I) x  (DESIGN.md section 3.5).
// R_s are the dense-slot kernel rows of a site set, already multiplied by sqrt(weight), stored LEVEL-MAJOR in one array
// rows_all[d][r][27].  Every site of a level-d cell c couples to the same 27 voxels (c's stencil):
//   t[r]     = sum_d sum_s rows[d][r][s] * x[nbr[c_d(r)][s]]
//   P[c][s]  = sum_{r in c} rows[d][r][s] * t[r],          y_j = reg x_j + sum_{s'} P[nbr[j][s']][26 - s']
// k_fz_cells makes P in ONE pass: t[r] needs only the row's own slots, so it is formed (one transposing butterfly per four rows) and
// used while the row is still in registers -- every kernel row is read from HBM once per application, there are no column indices,
// no t vector in memory and no second pass over the rows.
//
// The sweep walks UNITS, not rows.  A unit is a maximal run of rows that lie in the same cell at every level (in practice: the
// rows of one level-0 cell, ~4 of them); an item = the units that START in a 32-row window (item_begin[]: variable length, aligned to
// unit boundaries), one item per 32-lane half of a wavefront, lane = stencil slot.  Per trip a half-wave takes up to FZ_TRIP rows of
// its current unit: the stencil of the unit's level-0 cell is fetched once per UNIT (its neighbour row one unit ahead, so that
// every load of a trip is independent), level-0 blocks are always complete when their unit ends, and the coarser levels change
// cell only BETWEEN units -- no trip is ever cut.
//
// Where the blocks go.  A cell's block P[c][27] is final as soon as all rows of the cell have been seen:
//   * a cell that lies inside ONE workgroup's 256 rows is finished there: blocks of cells that cross an item boundary meet in LDS
//     at the end of the workgroup and are summed in item order (the exchange) -- only cells whose rows span several workgroups
//     (the coarse ones: ~1 % of the cells) leave partial blocks, one per workgroup, which k_fz_cellsum (csrc/fused.hip) adds;
//   * the per-cell sums are stored SLOT-MAJOR, ct[s][c], so that the gather runs with one lane per unknown; the blocks of a
//     workgroup's level-0 / level-1 cells are staged in LDS and leave in contiguous runs (fz_flush).
// Every summation order is fixed and depends on the rows' position inside their segment only (segments are padded to whole
// workgroups): no float atomics, deterministic, and a chunk's result does not depend on its batch mates.
//
// MODE 0: the operator (t from x).  MODE 1, the set-up pass: right-hand side (t = target) into ct / part, Jacobi diagonal
// (P2 += rows^2) into ct2 / part2, and the count of non-zero slots, all in one sweep over the rows.
//
// FAC, the factor form: the rows are not read but REBUILT -- the workgroup stages the 16-byte factor records of its ~256 rows in
// LDS (fz_stage_records), every cell change also fetches the psi stencil of the new cell next to its x stencil, and a trip turns
// records + stencil into the same w[u][d] the dense form loads (fz_rebuild_rows).  Everything downstream of w -- both products,
// blocks, exchange, staging -- is the dense form's code.
#include "fused_dev.h"
#include <type_traits>

// lane `l` of the caller's own half-wave, l uniform: two scalar lane reads + a select (no crossbar)
__device__ __forceinline__ int half_lane_i(int v, int l, bool upper) {
    const int lo = __builtin_amdgcn_readlane(v, l), hi = __builtin_amdgcn_readlane(v, 32 + l);
    return upper ? hi : lo;
}
__device__ __forceinline__ float half_lane_f(float v, int l, bool upper) { return __int_as_float(half_lane_i(__float_as_int(v), l, upper)); }

// ---- the LDS of a workgroup ----------------------------------------------------------------------------------------------------------
// The set-up pass keeps a SECOND block (the diagonal's) beside every block of b: second accumulators and LDS arrays are index
// [SECOND] of what the operator has one of, and every statement on them stands under `if (SETUP)`.
template <bool SETUP> struct FzSets { static constexpr int N = SETUP ? 2 : 1, SECOND = N - 1; };

// staging (st0, st1, stf in k_fz_cells): final blocks of the workgroup's level-0 / level-1 cells, staged so that they leave
// slot-major in contiguous runs (lane = cell): written word by word, 27 different lines per block, the per-cell sums cost the sweep
// 130 us of partial-line writes.  CAP0 / CAP1 blocks are staged: a workgroup holds ~64 / ~8 such cells at four rows per level-0 cell;
// more than fit are written word by word.
// (The set-up pass stages two arrays per block: at 96 / 32 blocks its 49.4 KB let three workgroups onto a CU, at 64 / 16 -- 38.9 KB --
// four.  With the count's atomic in the way that bought nothing, 15.4 against 14.8 ms; without it 11.4 against 12.6 ms.)
// (The staging and the exchange stay separate arrays, and two staging arrays: as members of one struct they share a base address,
// the compiler folds their index arithmetic, and the row loop of the operator is no longer the instruction stream that was measured.
// One merged staging array changed the instruction count of every instantiation.)
template <int D, bool SETUP> struct FzStage { static constexpr int CAP0 = SETUP ? 64 : 96, CAP1 = D > 1 ? (SETUP ? 16 : 32) : 1; };
template <int D, bool SETUP> using FzStaged0 = float[FzSets<SETUP>::N][FzStage<D, SETUP>::CAP0 * 27];
template <int D, bool SETUP> using FzStaged1 = float[FzSets<SETUP>::N][FzStage<D, SETUP>::CAP1 * 27];
// records (FAC): the factor records of the workgroup's rows.  FZ_RCAP rows are staged (a workgroup holds ~256; a unit that runs past
// this reads its records from memory) + four overflow slots per half-wave: the records of a trip past the staged window are copied
// there first
#define FZ_RCAP 288
template <int D, bool FAC = true> struct FzRecords {
    static constexpr int RS = FZ_RCAP + 4 * FZ_HW;
    float4 fv[FAC ? D * RS : 1], fp[FAC ? RS : 1];
};

// A workgroup WITHOUT rows: one unit (a cell with hundreds of sites) covers its whole 256-row window and belongs to the
// workgroup it starts in.  k_fz_block_counts gives a cell one partial block per workgroup from its first to its last, this
// one included, k_fz_cellsum adds them all, and the workspace has no initial value: the blocks nobody fills are written
// here, as zeros.  They belong to the coarse cells of the row before this workgroup (the covering unit's) that go on after it.
template <int D, bool SETUP>
__device__ __forceinline__ void fz_zero_uncovered(const FusedArgs& A, int W0, float* __restrict__ part, float* __restrict__ part2) {
    if (W0 > 0 && threadIdx.x < 32 * D) {
        const int d = threadIdx.x >> 5;
        const int c = A.row_cells[(int64_t)d * A.rows_total + W0 - 1];
        if (c >= 0 && A.nbr32[(int64_t)c * 32 + 29] >= W0) {
            const int64_t blk = (int64_t)A.nbr32[(int64_t)c * 32 + 27] + blockIdx.x;
            part[blk * 32 + (threadIdx.x & 31)] = 0.f;
            if (SETUP) part2[blk * 32 + (threadIdx.x & 31)] = 0.f;
        }
    }
    if (SETUP && A.nnz_counter && threadIdx.x == 0) A.nnz_counter[1 + blockIdx.x] = 0;     // (its entry has no initial value either)
}

// The staged blocks leave slot-major: lane = cell, 27 stores of contiguous runs.  cw0 / cw1: the first staged cell of level 0 / 1
template <int D, bool SETUP>
__device__ __forceinline__ void fz_flush(const FzStaged0<D, SETUP>& st0, const FzStaged1<D, SETUP>& st1, const int* stf, float* __restrict__ ct,
                                         float* __restrict__ ct2, int cw0, int cw1, int M) {
    constexpr int SECOND = FzSets<SETUP>::SECOND, CAP0 = FzStage<D, SETUP>::CAP0, CAP1 = FzStage<D, SETUP>::CAP1;
    const int t = threadIdx.x;
    const bool l0 = t < CAP0, l1 = !l0 && t < CAP0 + CAP1;
    if ((l0 || l1) && stf[t]) {
        const float* src = l0 ? st0[0] + t * 27 : st1[0] + (t - CAP0) * 27;
        const float* srcb = SETUP ? (l0 ? st0[SECOND] + t * 27 : st1[SECOND] + (t - CAP0) * 27) : nullptr;
        float* dst = ct + (l0 ? cw0 + t : cw1 + (t - CAP0));
        float* dstb = SETUP ? ct2 + (l0 ? cw0 + t : cw1 + (t - CAP0)) : nullptr;
#pragma unroll
        for (int q = 0; q < 27; ++q) {
            dst[(int64_t)q * M] = src[q];
            if (SETUP) dstb[(int64_t)q * M] = srcb[q];
        }
    }
}

// ---- factor form: the 27 slots of a row from its 16-byte records -----------------------------------------------------------------
// Quadratic B-spline weight of the centre at offset o - 1 for local coordinate u, written  a + b (u - c)^2  with per-lane constants
// (o = 0: 0.5 (1 - u)^2, 1: 0.75 - (u - 0.5)^2, 2: 0.5 u^2); its derivative is 2 b (u - c).  u = frac(p 2^-level) is exact: the
// level-d cell of a site is floor(p 2^-d), and p 2^-d - floor(p 2^-d) needs no rounding.
// (Measured and dropped: the same sums on v_mfma_f32_4x4x1 -- one quad lane per row, weights as a K = 2 polynomial product,
// dot products as K = 4: 65 matrix instructions per trip, 27.2 ms per application of the 64-chunk scene against 22.4 ms for
// this plain vector form at 7.3e9 VALU instructions; the dense-row sweep issues 2.3e9 and takes 11 ms.)
struct FzSpline { float a[3], b[3], c[3]; };      // per axis, for the lane's slot:  w(u) = a + b (u - c)^2,  dw/du = 2 b (u - c)
__device__ __forceinline__ FzSpline fz_spline_consts(int s) {
    FzSpline q;
    const int o[3] = {s / 9, (s / 3) % 3, s % 3};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {          // o = 0: 0.5 (1 - u)^2;  1: 0.75 - (u - 0.5)^2;  2: 0.5 u^2
        q.a[ax] = o[ax] == 1 ? 0.75f : 0.f;
        q.b[ax] = o[ax] == 1 ? -1.f : 0.5f;
        q.c[ax] = o[ax] == 0 ? 1.f : (o[ax] == 1 ? 0.5f : 0.f);
    }
    return q;
}
template <bool DER>
__device__ __forceinline__ void fz_axis(float p, float scale, float a, float b, float c, float k, float& w, float& dw) {
    const float u = __builtin_amdgcn_fractf(p * scale);
    const float t = u - c, bt = b * t;
    w = fmaf(bt, t, a);
    if (DER) dw = bt * k;
}
__device__ __forceinline__ float fz_dot4(const float4& a, const float4& b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

// The records of the workgroup's rows [W0, W1): (D + 1) coalesced bursts -- the only streaming loads of the FAC kernel -- all loads
// before the first store.  Rows past the last one (a trip reads four) are zeroed: never used (their t is 0) but they must be finite
template <int D>
__device__ __forceinline__ void fz_stage_records(const FusedArgs& A, int W0, int W1, FzRecords<D>& R) {
    const int nw = W1 - W0 < FZ_RCAP ? W1 - W0 : FZ_RCAP;
    if (nw > 0) {
        const int t0 = threadIdx.x, t1 = threadIdx.x + FZ_BLOCK;
        float4 v0[D + 1], v1[D + 1];
#pragma unroll
        for (int d = 0; d <= D; ++d) {
            const float4* src = (d < D ? A.fac_vec + (int64_t)d * A.rows_total : A.fac_pos) + W0;
            v0[d] = src[t0 < nw ? t0 : nw - 1];
            v1[d] = src[t1 < nw ? t1 : nw - 1];
        }
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int d = 0; d <= D; ++d) {
            float4* dst = d < D ? R.fv + d * R.RS : R.fp;
            if (t0 < nw + 4 && t0 < FZ_RCAP) dst[t0] = t0 < nw ? v0[d] : zero;
            if (t1 < nw + 4 && t1 < FZ_RCAP) dst[t1] = t1 < nw ? v1[d] : zero;
        }
    }
}

// A trip's rows r .. r + 3 from their records and the psi stencils ps[] of the current cells:
//   position rows (<= 4 per trip):   w = B_s(u) <phi, psi_s>
//   a normal site (header + 3 rows): w_a = <phi, psi_s> dB_s/dx_a + <J_a, psi_s> B_s    (B, dB shared by the three rows)
// A trip is EITHER a run of position rows OR one normal site (always inside one unit): nt is cut to the rows it holds.
template <int D, bool SETUP>
__device__ __forceinline__ void fz_rebuild_rows(const FusedArgs& A, FzRecords<D>& R, const FzSpline& bq, float4 (&ps)[D], bool live0, const float4& pg,
                                                int r, int W0, int hwi, int s, bool act, int& nt, float (&w)[FZ_TRIP][D]) {
    constexpr int U = FZ_TRIP, RS = FzRecords<D>::RS;
    // the records of rows r .. r + 3 from LDS (all lanes of the half-wave read the same address: a broadcast)
    int rl = r - W0;
    if (rl + U > FZ_RCAP) {
        // (rare: a unit that runs past the staged window -- a cell with dozens of points: its records are copied to the
        // half-wave's four overflow slots first)
        rl = FZ_RCAP + 4 * hwi;
        if (s < 4) {
            R.fp[rl + s] = A.fac_pos[(int64_t)r + s];
#pragma unroll
            for (int d = 0; d < D; ++d) R.fv[d * RS + rl + s] = A.fac_vec[(int64_t)d * A.rows_total + r + s];
        }
        __builtin_amdgcn_wave_barrier();                  // (lanes s < 4 write, every lane of the half-wave reads)
    }
    float4 pq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) pq[u] = R.fp[rl + u];
    const bool site = __float_as_int(pq[0].w) == 1;
    const bool q1 = __float_as_int(pq[1].w) == 0, q2 = q1 && __float_as_int(pq[2].w) == 0, q3 = q2 && __float_as_int(pq[3].w) == 0;
    const int np = site ? U : 1 + (q1 ? 1 : 0) + (q2 ? 1 : 0) + (q3 ? 1 : 0);
    nt = nt < np ? nt : np;
    ps[0] = live0 ? pg : make_float4(0.f, 0.f, 0.f, 0.f);         // the psi stencil of the unit's level-0 cell (pg: as loaded, unmasked)
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float scale = __int_as_float((127 - d) << 23);          // 2^-d
        const float k2 = 2.f * A.inv_w0 * scale;                       // 2 / w_d
        float4 vq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) vq[u] = R.fv[d * RS + rl + u];
        if (site) {
            float wx, wy, wz, dx, dy, dz;
            fz_axis<true>(pq[0].x, scale, bq.a[0], bq.b[0], bq.c[0], k2, wx, dx);
            fz_axis<true>(pq[0].y, scale, bq.a[1], bq.b[1], bq.c[1], k2, wy, dy);
            fz_axis<true>(pq[0].z, scale, bq.a[2], bq.b[2], bq.c[2], k2, wz, dz);
            const float yz = wy * wz, B = wx * yz;
            const float g = fz_dot4(vq[0], ps[d]);
            w[0][d] = 0.f;
            w[1][d] = fmaf(fz_dot4(vq[1], ps[d]), B, g * (dx * yz));
            w[2][d] = fmaf(fz_dot4(vq[2], ps[d]), B, g * ((wx * wz) * dy));
            w[3][d] = fmaf(fz_dot4(vq[3], ps[d]), B, g * ((wx * wy) * dz));
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float wx, wy, wz, unused;
                fz_axis<false>(pq[u].x, scale, bq.a[0], bq.b[0], bq.c[0], 0.f, wx, unused);
                fz_axis<false>(pq[u].y, scale, bq.a[1], bq.b[1], bq.c[1], 0.f, wy, unused);
                fz_axis<false>(pq[u].z, scale, bq.a[2], bq.b[2], bq.c[2], 0.f, wz, unused);
                w[u][d] = fz_dot4(vq[u], ps[d]) * (wx * (wy * wz));
            }
        }
    }
    if (SETUP && A.dense_out) {
        // the coarse-level block of the preconditioner is assembled from DENSE rows: the levels it covers leave here
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d >= A.dense_from && act)
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < nt) A.dense_out[((int64_t)(d - A.dense_from) * A.rows_total + r + u) * 27 + s] = w[u][d];
    }
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------------------
template <int MODE, int D, bool FAC>
__global__ void __attribute__((amdgpu_waves_per_eu(FAC ? 3 : (D <= 4 ? 6 : 5)))) __launch_bounds__(FZ_BLOCK) k_fz_cells(FusedArgs A, const float* __restrict__ x, float* __restrict__ part,
                                                      float* __restrict__ part2, float* __restrict__ ct, float* __restrict__ ct2,
                                                      const int* __restrict__ done) {
    if (done && *done) return;
    constexpr bool SETUP = MODE == 1;
    constexpr int U = FZ_TRIP, SECOND = FzSets<SETUP>::SECOND;
    // exchange: blocks of coarse cells that cross an item boundary inside this workgroup: [item][level][0: the item's first cell, which
    // began before it / 1: its last cell, which goes on after it] -- summed after the row loop (see below)
    __shared__ float xv[FzSets<SETUP>::N][FZ_HW][D][2][32];
    __shared__ int xm[FZ_HW][D][2];                                  // their cells (-1: no entry; bit 30: the cell ends in that item)
    __shared__ int xmb[FZ_HW][D][2];                                 // their block bases
    __shared__ int xbase[FZ_HW][D];                                  // block base of the current cell of every level
    __shared__ int wnnz[FZ_BLOCK / 64];                              // SETUP: the non-zero slots every wavefront saw
    constexpr int CAP0 = FzStage<D, SETUP>::CAP0, CAP1 = FzStage<D, SETUP>::CAP1;
    __shared__ FzStaged0<D, SETUP> st0;                              // staging: the final blocks of the first CAP0 level-0 cells,
    __shared__ FzStaged1<D, SETUP> st1;                              // of the first CAP1 level-1 cells,
    __shared__ int stf[CAP0 + CAP1];                                 // and which of them are filled
    __shared__ FzRecords<D, FAC> R;                                  // records (FAC)
    for (int i = threadIdx.x; i < CAP0 + CAP1; i += FZ_BLOCK) stf[i] = 0;
    const int W0 = __builtin_amdgcn_readfirstlane(A.item_begin[blockIdx.x * FZ_HW]);
    if (__builtin_amdgcn_readfirstlane(A.item_begin[(blockIdx.x + 1) * FZ_HW]) == W0) {
        fz_zero_uncovered<D, SETUP>(A, W0, part, part2);
        return;
    }
    if constexpr (FAC) {
        const int W1 = __builtin_amdgcn_readfirstlane(A.item_begin[(blockIdx.x + 1) * FZ_HW]);
        if (MODE == 0 && W1 > W0 && fz_seg_done(A, A.item_seg, W0 >> 5)) return;      // (a workgroup lies inside ONE segment)
        fz_stage_records<D>(A, W0, W1, R);
    }
    __syncthreads();
    const int hwi = threadIdx.x >> 5;
    const int item = blockIdx.x * FZ_HW + hwi;
    const int s = threadIdx.x & 31;
    const bool act = s < 27, upper = (threadIdx.x & 32) != 0;
    const int sh = upper ? 32 : 0;
    const int sc = act ? s : 26;
    const int Rb = A.item_begin[item];                               // (row numbers fit an int: rows_total < 2^31 - 512)
    int Re = A.item_begin[item + 1];
    // (the rows of a segment whose conjugate gradients have finished are skipped: a workgroup lies inside ONE segment -- segments
    // are padded to whole workgroups)
    if (MODE == 0 && Re > Rb && fz_seg_done(A, A.item_seg, Rb >> 5)) Re = Rb;
    // first cell of the staged levels with rows in this workgroup (uniform)
    const int cw0 = __builtin_amdgcn_readfirstlane((int64_t)W0 < A.rows_total ? A.row_cells[W0] : -1);
    const int cw1 = __builtin_amdgcn_readfirstlane((D > 1 && (int64_t)W0 < A.rows_total) ? A.row_cells[A.rows_total + W0] : -1);
    if (s < 2 * D) xm[hwi][s >> 1][s & 1] = -1;
    // the cells of the item's first 32 rows, one row per lane (every unit of the item starts among them)
    const int len32 = Re - Rb < 32 ? Re - Rb : 32;
    int cells[D];
    unsigned chg[D > 1 ? D : 2];     // levels >= 1, bit l: row l lies in another cell than row l - 1
    unsigned um = 0;                 // bit l: a unit starts at row l
#pragma unroll
    for (int d = 0; d < D; ++d) {
        cells[d] = s < len32 ? A.row_cells[(int64_t)d * A.rows_total + Rb + s] : -1;
        const int before = __shfl_up(cells[d], 1, 32);
        const unsigned m = (unsigned)(__ballot(s > 0 && s < len32 && cells[d] != before) >> sh);
        if (d > 0) chg[d] = m;
        um |= m;
    }
    um |= 1u;
    // of the current cell of every coarse level two bits are kept: do its rows start / end inside this item (bits 2 d, 2 d + 1)
    unsigned inside = 0;
    float P[FzSets<SETUP>::N][D], xs[D];         // P[0]: the running block of every level;  P[SECOND]: the diagonal's (SETUP)
    bool have[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { P[0][d] = 0.f; P[SECOND][d] = 0.f; xs[d] = 0.f; have[d] = false; }
    // nbv: the neighbour row of the cell that becomes current at level d (lanes 27 / 28 / 29: its block base, first / last row)
    auto enter = [&](int d, int nbv) {
        const int first = __shfl(nbv, 28, 32), last = __shfl(nbv, 29, 32);
        if (s == 27) xbase[hwi][d] = nbv;
        inside = (inside & ~(3u << (2 * d))) | ((first >= Rb ? 1u : 0u) << (2 * d)) | ((last < Re ? 2u : 0u) << (2 * d));
    };
    // the final block of a cell that lies inside this workgroup: staged (levels 0 and 1, while there is room) or written word by word
    auto finish = [&](int d, int cell, float p, float p2) {
        const int rel = d == 0 ? cell - cw0 : cell - cw1;
        if (d == 0 && cw0 >= 0 && (unsigned)rel < (unsigned)CAP0) {
            if (act) { st0[0][rel * 27 + s] = p; if (SETUP) st0[SECOND][rel * 27 + s] = p2; }
            if (s == 0) stf[rel] = 1;
        } else if (d == 1 && cw1 >= 0 && (unsigned)rel < (unsigned)CAP1) {
            if (act) { st1[0][rel * 27 + s] = p; if (SETUP) st1[SECOND][rel * 27 + s] = p2; }
            if (s == 0) stf[CAP0 + rel] = 1;
        } else if (act) {
            ct[(int64_t)s * A.M + cell] = p;
            if (SETUP) ct2[(int64_t)s * A.M + cell] = p2;
        }
    };
    // the running block of coarse level d leaves (`cell`: its cell): complete (all rows of the cell lie in this item) -> final;
    // otherwise -> the workgroup exchange
    auto emit = [&](int d, int cell, float p, float p2) {
        const unsigned f = (inside >> (2 * d)) & 3u;
        if (f == 3u) {
            finish(d, cell, p, p2);
        } else {
            const int k = (int)(f & 1u);
            xv[0][hwi][d][k][s] = p;
            if (SETUP) xv[SECOND][hwi][d][k][s] = p2;
            if (s == 0) { xm[hwi][d][k] = cell | ((f & 2u) ? (1 << 30) : 0); xmb[hwi][d][k] = xbase[hwi][d]; }
        }
    };
    // end row of the unit that starts at position p (of the item's first 32 rows)
    auto unit_end = [&](int p) {
        const unsigned after = um & ~((2u << p) - 1u);
        return after ? Rb + (int)__builtin_ctz(after) : Re;
    };
    // ---- the first unit: its stencils at all levels (one round trip for the neighbour rows, one for x)
    bool work = Rb < Re;
    int pos = 0, r = Rb, uend = unit_end(0);
    // one pointer per level (slot s of row 0), the U rows of a trip at immediate offsets.  Rows past the unit's (or the item's) last
    // one are read too (the rows that follow: the array is padded) and never used: their t is 0
    const float* wp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) wp[d] = FAC ? nullptr : A.rows_all + (int64_t)d * A.rows_total * 27 + sc;
    int c0 = __shfl(cells[0], 0, 32);
    int line0;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ps[D];                                                    // FAC: the psi stencil of the current cell of every level
    {
        int cd[D], nb0[D];
        float x0[D];
        float4 p0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            cd[d] = __shfl(cells[d], 0, 32);
            nb0[d] = A.nbr32[(int64_t)(cd[d] >= 0 ? cd[d] : 0) * 32 + s];
        }
#pragma unroll
        for (int d = 1; d < D; ++d) {
            x0[d] = MODE == 0 ? x[(act && nb0[d] >= 0) ? nb0[d] : 0] : 0.f;
            if (FAC) p0[d] = A.psi_all[(act && nb0[d] >= 0) ? nb0[d] : 0];
        }
        line0 = nb0[0];
#pragma unroll
        for (int d = 1; d < D; ++d) {
            have[d] = work && cd[d] >= 0;
            enter(d, nb0[d]);
            xs[d] = (have[d] && act && nb0[d] >= 0) ? x0[d] : 0.f;
            if (FAC) ps[d] = (have[d] && act && nb0[d] >= 0) ? p0[d] : zero4;
        }
        if (FAC) ps[0] = zero4;
    }
    const FzSpline bq = fz_spline_consts(sc);
    int nnz = 0;                                                     // MODE 1: this lane's non-zero slots (stored entries of G and Q)
    while (__any(work)) {
        // all loads of the trip: U rows x D levels, the x stencil of the unit's level-0 cell, the neighbour row of the NEXT unit's
        // level-0 cell (all unconditional -- clamped addresses, results masked afterwards: a load under a branch makes the compiler
        // lose count of the outstanding loads and wait for all of them).  Plain loads: with the non-temporal hint the sweep was
        // 9-13 % SLOWER -- a 108-byte row shares its cache lines with its neighbours in the list, which the four rows of a trip and
        // the next trip fetch again
        float w[U][D];
        if (!FAC) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int d = 0; d < D; ++d) w[u][d] = *(wp[d] + ((int64_t)r + u) * 27);
        }
        const float xg = MODE == 0 ? x[(act && line0 >= 0) ? line0 : 0] : 0.f;
        float4 pg = zero4;
        if (FAC) pg = A.psi_all[(act && line0 >= 0) ? line0 : 0];
        float tg[U];
        if (MODE == 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) tg[u] = A.targets_all ? A.targets_all[r + u] : 0.f;       // (targets_all is padded like the rows)
        }
        const int npos = uend - Rb;                                   // the next unit starts here, if the item goes on
        const int cn = __shfl(cells[0], npos & 31, 32);
        const int line0n = A.nbr32[(int64_t)((uend < Re && cn >= 0) ? cn : 0) * 32 + s];
        int nt = work ? (uend - r < U ? uend - r : U) : 0;            // rows of this trip
        if constexpr (FAC) {
            fz_rebuild_rows<D, SETUP>(A, R, bq, ps, c0 >= 0 && act && line0 >= 0, pg, r, W0, hwi, s, act, nt, w);
        }
        const float x0 = (c0 >= 0 && act && line0 >= 0) ? xg : 0.f;
        float t[U];
        if (MODE == 0) {
            float prod[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                prod[u] = w[u][0] * x0;
#pragma unroll
                for (int d = 1; d < D; ++d) prod[u] = fmaf(w[u][d], xs[d], prod[u]);
            }
            const float rs = half_sum4(prod[0], prod[1], prod[2], prod[3], s);
#pragma unroll
            for (int u = 0; u < U; ++u) t[u] = u < nt ? half_lane_f(rs, 8 * u, upper) : 0.f;
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = u < nt && act;
                t[u] = u < nt ? tg[u] : 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) { w[u][d] = ok ? w[u][d] : 0.f; nnz += w[u][d] != 0.f ? 1 : 0; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                P[0][d] = fmaf(w[u][d], t[u], P[0][d]);
                if (SETUP) P[SECOND][d] = fmaf(w[u][d], w[u][d], P[SECOND][d]);
            }
        r += nt;
        if (work && r >= uend) {
            // the unit is done: its level-0 block is final
            if (c0 >= 0) finish(0, c0, P[0][0], P[SECOND][0]);
            P[0][0] = 0.f;
            if (SETUP) P[SECOND][0] = 0.f;
            work = uend < Re;
            if (work) {
                pos = npos;
                c0 = cn;
                line0 = line0n;
                uend = unit_end(pos);
                // coarse levels whose cell changes with this unit: the finished block leaves, the new stencil is fetched (rare: a
                // level-1 cell holds ~8 units)
#pragma unroll
                for (int d = 1; d < D; ++d)
                    if ((chg[d] >> pos) & 1u) {
                        const int before = __shfl(cells[d], (pos + 31) & 31, 32);
                        if (have[d]) emit(d, before, P[0][d], P[SECOND][d]);
                        P[0][d] = 0.f;
                        if (SETUP) P[SECOND][d] = 0.f;
                        xs[d] = 0.f;
                        if (FAC) ps[d] = zero4;
                        const int cd = __shfl(cells[d], pos, 32);
                        have[d] = cd >= 0;
                        if (have[d]) {
                            const int nbv = A.nbr32[(int64_t)cd * 32 + s];
                            enter(d, nbv);
                            if (MODE == 0 && act && nbv >= 0) xs[d] = x[nbv];
                            if (FAC && act && nbv >= 0) ps[d] = A.psi_all[nbv];
                        }
                    }
            }
        }
    }
#pragma unroll
    for (int d = 1; d < D; ++d)
        if (have[d]) emit(d, __shfl(cells[d], pos, 32), P[0][d], P[SECOND][d]);
    // the count leaves as ONE plain store per workgroup (an atomicAdd per wavefront on one word -- 1.09 M of them in the scene's
    // sweep -- ran at the rate the memory system serialises them)
    if (SETUP && A.nnz_counter) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nnz += __shfl_xor(nnz, o);
        if ((threadIdx.x & 63) == 0) wnnz[threadIdx.x >> 6] = nnz;
    }
    // ---- coarse cells that cross item boundaries inside this workgroup: the LAST item of the workgroup that holds a piece of the cell
    // adds the pieces in item order.  A cell that lies inside the workgroup is final; one that reaches into other workgroups leaves
    // one partial block per workgroup (k_fz_cellsum adds those).  Everything is decided from the exchange in LDS: an item holds a
    // piece of cell c <=> one of its two entries names c; a cell began in the item that holds it as its LAST cell (entry 1); items
    // may be empty (a long unit covers their window).  (Inline: as a function of its own this block changed the order of the row
    // loop's instructions at depths 2, 4 and 6.)
    __syncthreads();
    if (SETUP && A.nnz_counter && threadIdx.x == 0) {
        unsigned long long tot = 0;
#pragma unroll
        for (int q = 0; q < FZ_BLOCK / 64; ++q) tot += (unsigned long long)wnnz[q];
        A.nnz_counter[1 + blockIdx.x] = tot;
    }
#pragma unroll
    for (int d = 1; d < D; ++d)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = xm[hwi][d][k];
            if (e < 0) continue;
            const int c = e & ~(1 << 30);
            const bool ends = (e >> 30) & 1;
            bool later = false;
            if (!ends)
                for (int h = hwi + 1; h < FZ_HW; ++h) later = later || (xm[h][d][0] >= 0 && (xm[h][d][0] & ~(1 << 30)) == c);
            if (later) continue;
            int h0 = hwi;
            bool started = k == 1;
            while (!started && h0 > 0) {
                --h0;
                started = xm[h0][d][1] >= 0 && (xm[h0][d][1] & ~(1 << 30)) == c;
            }
            float acc = 0.f, acc2 = 0.f;
            for (int h = h0; h <= hwi; ++h) {
                const int kk = (h == h0 && started) ? 1 : 0;
                const int eh = h == hwi ? e : xm[h][d][kk];
                if (eh < 0 || (eh & ~(1 << 30)) != c) continue;       // (an empty item in between)
                acc += xv[0][h][d][kk][s];
                if (SETUP) acc2 += xv[SECOND][h][d][kk][s];
            }
            if (started && ends) {
                finish(d, c, acc, acc2);
            } else {
                const int base = xmb[hwi][d][k];
                part[((int64_t)base + blockIdx.x) * 32 + s] = acc;
                if (SETUP) part2[((int64_t)base + blockIdx.x) * 32 + s] = acc2;
            }
        }
    __syncthreads();
    fz_flush<D, SETUP>(st0, st1, stf, ct, ct2, cw0, cw1, A.M);
}

// f(std::integral_constant<int, N>) with N = depth clamped to [1, MAX]: the run-time depth as a template argument
template <int MAX, class F>
static inline void fz_with_depth(int depth, F&& f) {
    if constexpr (MAX > 1) {
        if (depth < MAX) return fz_with_depth<MAX - 1>(depth, f);
    }
    f(std::integral_constant<int, MAX>{});
}

template <int MODE>
void fz_sweep(const FusedArgs& A, const float* x, const FusedWork& w, const int* done, hipStream_t st) {
    if (A.hw_total <= 0) return;
    const dim3 grid(nksr_blocks((int64_t)A.hw_total, FZ_HW)), blk(FZ_BLOCK);
    fz_with_depth<NKSR_MAX_DEPTH>(A.depth, [&](auto depth) {
        constexpr int D = decltype(depth)::value;
        if (A.fac_vec) hipLaunchKernelGGL((k_fz_cells<MODE, D, true>), grid, blk, 0, st, A, x, w.part, w.part2, w.ct, w.ct2, done);
        else hipLaunchKernelGGL((k_fz_cells<MODE, D, false>), grid, blk, 0, st, A, x, w.part, w.part2, w.ct, w.ct2, done);
    });
}
template void fz_sweep<0>(const FusedArgs&, const float*, const FusedWork&, const int*, hipStream_t);
template void fz_sweep<1>(const FusedArgs&, const float*, const FusedWork&, const int*, hipStream_t);
