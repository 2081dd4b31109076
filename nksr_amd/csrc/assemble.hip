// Normal-equation assembly  A = sum_s w_s R_s^T R_s + reg I,  b = sum_s w_s R_s^T t_s
// (KernelField.solve_non_fused, reference call site models/nksr_net.py:105-112).
//
// Design -- two phases, no float atomics, fixed summation order:
//  1. cell blocks (csrc/gram.hip).  All sites (input points / normal samples) inside one level-d cell c share
//     their 27-voxel stencil at every level >= d, so their joint contribution is one dense
//     block  B[d][c] = sum_k w r_k[d][0:27]^T r_k[d:L][0:27]   of shape 27 x T_d, T_d = 27 (L-d), formed on the matrix cores.
//     Levels >= 3 split: a cell of R rows is summed in min(asm_level_parts(d), R / 128) parts, and the schedule of the parts --
//     one wavefront per (cell, part) or one per cell -- is picked by the level's size, with the same bits either way.
//  2. structure.  k_row_count maps every structural upper slot of a row (column voxel exists and
//     the two B-spline supports overlap: integer test) to its column (colmap), counts them and
//     accumulates the in-degree of every destination row with INTEGER atomics (order-independent).
//     Exclusive scans then give the final row pointers: row = [mirrors][own upper][diagonal].
//  3. row gather.  Row i (voxel at level d) adds, for each of its 27 neighbour cells c, the block
//     row B[d][c][slot of i in c's stencil] into a structured (L-d) x 5^3 slot frame in LDS (row_gather) and
//     writes its own upper entries + diagonal straight into their final CSR slots; the mirrored
//     copies go to a list keyed by destination row (emit_csr).
//  4. a STABLE radix sort of that list on the destination-row bits (3 passes over HALF of the
//     entries) orders every row's mirrors by ascending source row; k_place_mirrors drops them into
//     the CSR.  Deterministic and exactly symmetric, no float atomics, no full COO.
//  The coarse-level block of the PCG's preconditioner, when it is stored packed (csrc/cheb.hip, format 1), skips the CSR: steps 3 and 4
//  become  3'. k_row_diag (every diagonal, ahead of the fill) + the fill with the drop test inside (emit_packed: kept entries leave as
//  packed words),  4'. the kept mirror words alone compacted, sorted keys-only, and one kernel that writes the packed rows
//  (csrc/packed_rows.hip) -- "the packed coarse block straight from the slot frame" below, nksr_assemble_packed in include/nksr_hip.h.
#include "assemble_dev.h"
#include "coarse_pack_dev.h"
#include <stdlib.h>

// ---- phase 2a: structure.  colmap[row slot] = column of every structural slot ---------------------------
// One wavefront walks RC_RUN Morton-consecutive rows.  Such rows share their coarse ancestors, hence the
// 5^3 column frames of the coarser levels: a frame (125 hash lookups) is fetched when the ancestor changes
// and stays in REGISTERS -- lane l owns frame slots l and l + 64, together with the number of rows of the
// run that coupled to them, which becomes ONE global integer atomic per touched column when the frame is
// retired (instead of one per structural entry).  No LDS, no barriers, no float atomics; integer
// atomics are order-independent, so the result is deterministic.
// Frame slots run x fastest (slot = (z * 5 + y) * 5 + x): the unknowns of a level are Morton-ordered with x in the lowest bit, so the
// voxels (2k, y, z), (2k + 1, y, z) have CONSECUTIVE indices and land on adjacent frame slots -- a row's entries then come out with
// consecutive columns next to each other (the SpMV's x gathers of one 64-entry group then touch fewer 64-byte segments).
// colmap encoding: upper neighbour -> column, same-level lower neighbour -> -2 - column (emitted by the
// row itself: bitwise equal to the transposed entry), diagonal / absent / non-overlapping -> -1.
#define RC_RUN 32
__global__ void __launch_bounds__(ASM_WAVES * 64) k_row_count(AsmArgs A, int32_t* __restrict__ rowcount,
                                                              int32_t* __restrict__ crosscount, int32_t* __restrict__ samelow,
                                                              int32_t* __restrict__ indeg) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const nksr_hier_t& h = A.hier;
    const int L = h.depth;
    const int row0 = (blockIdx.x * ASM_WAVES + wave) * RC_RUN;
    if (row0 >= A.M) return;
    constexpr int F = NKSR_MAX_DEPTH - 1;
    int cf[F][2], nf[F][2];                 // frame dd (index dd - 1): columns and coupling counts of slots lane, lane + 64
    int kd[F], kx[F], ky[F], kz[F];         // ancestor the cached frame belongs to (kd < 0: none)
#pragma unroll
    for (int f = 0; f < F; ++f) { kd[f] = -1; kx[f] = ky[f] = kz[f] = 0; cf[f][0] = cf[f][1] = -1; nf[f][0] = nf[f][1] = 0; }
    const int r1 = lane + 64 < 125 ? lane + 64 : 124;       // second slot of the lane (lanes 61..63 idle there)
    const bool has1 = lane + 64 < 125;

    for (int row = row0; row < row0 + RC_RUN && row < A.M; ++row) {
        const int d = row_level(h, row);
        const nksr_level_t& lv0 = h.lv[d];
        const int i = row - lv0.offset;
        const int ix = lv0.ijk[i * 3], iy = lv0.ijk[i * 3 + 1], iz = lv0.ijk[i * 3 + 2];
        const int nslots = (L - d) * 125;
        int32_t* cm = A.colmap[d] + (int64_t)i * nslots;
        int cnt = 0, lower = 0, cross = 0;

        // coarser levels: (re)load the frames whose ancestor changed, retiring the old ones
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int dd = f + 1;
            if (d + dd >= L) continue;
            const int ax = ix >> dd, ay = iy >> dd, az = iz >> dd;
            if (kd[f] == d && kx[f] == ax && ky[f] == ay && kz[f] == az) continue;
            if (kd[f] >= 0) {
                if (nf[f][0] > 0) atomicAdd(&indeg[cf[f][0]], nf[f][0]);
                if (nf[f][1] > 0) atomicAdd(&indeg[cf[f][1]], nf[f][1]);
            }
            const nksr_level_t& lc = h.lv[d + dd];
            const int bias = NKSR_BIAS0 >> (d + dd);
            int j0 = hash_find(lc.hkeys, lc.hvals, lc.hcap, morton_biased(ax + lane % 5 - 2, ay + (lane / 5) % 5 - 2, az + lane / 25 - 2, bias));
            int j1 = has1 ? hash_find(lc.hkeys, lc.hvals, lc.hcap, morton_biased(ax + r1 % 5 - 2, ay + (r1 / 5) % 5 - 2, az + r1 / 25 - 2, bias)) : -1;
            cf[f][0] = j0 < 0 ? -1 : lc.offset + j0;
            cf[f][1] = j1 < 0 ? -1 : lc.offset + j1;
            nf[f][0] = nf[f][1] = 0;
            kd[f] = d; kx[f] = ax; ky[f] = ay; kz[f] = az;
        }

        // same level: the 5^3 frame through the 27-neighbour table -- slot (dx,dy,dz), |d| <= 2, is neighbour
        // (d - e) of neighbour e = clamp(d, -1, 1): two reads inside 108-byte table rows that Morton-adjacent
        // matrix rows share, instead of a random hash probe per slot; the hash is only consulted when the
        // intermediate voxel does not exist.  Every slot of this frame overlaps (|dI| <= 2).
        const int nb_lane = (lane < 27) ? lv0.nbr[(int64_t)i * 27 + lane] : -1;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = u == 0 ? lane : r1;
            const bool on = u == 0 || has1;
            const int dx = r % 5 - 2, dy = (r / 5) % 5 - 2, dz = r / 25 - 2;          // frame slot r = (z, y, x), x fastest
            const int ex = dx < -1 ? -1 : (dx > 1 ? 1 : dx), ey = dy < -1 ? -1 : (dy > 1 ? 1 : dy), ez = dz < -1 ? -1 : (dz > 1 ? 1 : dz);
            const int n1 = __shfl(nb_lane, (ex + 1) * 9 + (ey + 1) * 3 + (ez + 1));
            int col = -1;
            if (on) {
                int j;
                if (n1 >= 0) j = lv0.nbr[(int64_t)n1 * 27 + (dx - ex + 1) * 9 + (dy - ey + 1) * 3 + (dz - ez + 1)];
                else j = hash_find(lv0.hkeys, lv0.hvals, lv0.hcap, morton_biased(ix + dx, iy + dy, iz + dz, NKSR_BIAS0 >> d));
                col = j < 0 ? -1 : lv0.offset + j;
            }
            const bool lo = col >= 0 && col < row;
            lower += __popcll(__ballot(lo));
            if (col == row) col = -1;
            cnt += __popcll(__ballot(col > row));
            if (on) cm[r] = lo ? -2 - col : col;
        }

        // coarser levels: integer support-overlap test  |(2I+1) - (2J+1) 2^dd| < 3 (1 + 2^dd)  on every axis
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int dd = f + 1;
            if (d + dd >= L) continue;
            const int lim = 3 * (1 + (1 << dd));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = u == 0 ? lane : r1;
                const bool on = u == 0 || has1;
                const int x = (ix >> dd) + r % 5 - 2, y = (iy >> dd) + (r / 5) % 5 - 2, z = (iz >> dd) + r / 25 - 2;
                const int ox = (2 * ix + 1) - ((2 * x + 1) << dd), oy = (2 * iy + 1) - ((2 * y + 1) << dd),
                          oz = (2 * iz + 1) - ((2 * z + 1) << dd);
                int col = -1;
                if (on && abs(ox) < lim && abs(oy) < lim && abs(oz) < lim) col = cf[f][u];
                if (on) cm[dd * 125 + r] = col;
                if (col >= 0) nf[f][u] += 1;
                cross += __popcll(__ballot(col >= 0));
            }
        }
        if (lane == 0) {
            rowcount[row] = cnt + cross;
            crosscount[row] = cross;
            samelow[row] = lower;
        }
    }
    // retire the frames that are still cached
#pragma unroll
    for (int f = 0; f < F; ++f) {
        if (kd[f] < 0) continue;
        if (nf[f][0] > 0) atomicAdd(&indeg[cf[f][0]], nf[f][0]);
        if (nf[f][1] > 0) atomicAdd(&indeg[cf[f][1]], nf[f][1]);
    }
}

// NQ consecutive floats per lane from a 4-byte aligned block row: ONE vector-memory instruction per row
// (a row fill issues ~100 of them per matrix row and each costs ~16 clocks in the CU's address unit)
template <int NQ> struct cols_u { float v[NQ]; } __attribute__((packed, aligned(4)));
template <int NQ>
__device__ __forceinline__ void load_cols(const float* __restrict__ row, int lane, int T, float out[NQ]) {
    const int t0 = NQ * lane;
    if (t0 + NQ <= T) {
        const cols_u<NQ> c = *reinterpret_cast<const cols_u<NQ>*>(row + t0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) out[q] = c.v[q];
    } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) out[q] = (t0 + q < T) ? row[t0 + q] : 0.f;
    }
}

// ---- the packed coarse block straight from the slot frame (nksr_assemble_packed) ---------------------------------------------------
// The preconditioner's block is stored Jacobi-scaled in half precision with the entries below `drop` of the unit diagonal left out
// (csrc/cheb.hip, format 1): a row is assembled with ~250 entries and keeps ~37.  The drop test of entry (i, j) needs nothing the fill
// does not hold except the diagonal of row j, and that is ONE element of each of the 27 neighbour cells' blocks: k_row_diag forms all
// diagonals ahead of the fill (same terms, same order, same bits), and the fill (PACK) emits only what survives --
//   own entries (same-level lower, own upper) as final packed words  half << 16 | column local to the segment,  compacted inside the
//     row's structural range [own_off[row], own_off[row + 1]): the lower run from its start, the upper run from + samelow[row];
//   the mirror of a kept cross-level entry as one 64-bit word  destination row (new order) << 32 | half << 16 | local column of the
//     SOURCE row,  compacted inside [mir_off[row], mir_off[row + 1]);
//   kept[0 / 1 / 2][row] = kept lower / upper / mirror entries.
// csrc/packed_rows.hip makes the rows of these words.  The drop rule and the 32-bit word are those of coarse_pack_dev.h, which the
// converter of the fp32 CSR (csrc/cheb.hip) includes too.

struct AsmPackOut {
    const float* diag;          // [M] from k_row_diag
    const int32_t* new_of_old;  // [M] segment-major renumbering
    const int32_t* local;       // [M] new_of_old[row] - seg_base[segment of row]
    const int32_t* own_off;     // [M + 1] exclusive scan of samelow + rowcount
    uint32_t* own;              // kept own words
    uint64_t* mir;              // kept mirror words
    int32_t* kept;              // [3][M + 1]
    float drop;
};

// diag[row] = acc[62] + reg of the fill: the block element (row 26 - s, column 26 - s) of every neighbour cell s that holds sites, added
// in ascending s from 0.f -- the order of the fill's batches.  32 lanes per row.
__global__ void __launch_bounds__(256) k_row_diag(AsmArgs A, float* __restrict__ diag) {
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 5, l = threadIdx.x & 31;
    if (row >= A.M) return;
    const nksr_hier_t& h = A.hier;
    const int d = row_level(h, row);
    const nksr_level_t& lv = h.lv[d];
    const int i = row - lv.offset;
    const int T = (h.depth - d) * 27;
    const int c = (l < 27) ? lv.nbr[(int64_t)i * 27 + l] : -1;
    const int on = (c >= 0 && A.nsites[d][c] > 0) ? 1 : 0;
    const float x = on ? A.blocks[d][((int64_t)c * 27 + (26 - l)) * T + (26 - l)] : 0.f;
    float s = 0.f;
    for (int sp = 0; sp < 27; ++sp) {
        const float v = __shfl(x, sp, 32);
        if (__shfl(on, sp, 32)) s += v;
    }
    if (l == 0) diag[row] = s + A.reg;
}

// ---- phase 2b: one wavefront per row: gather block rows into the slot frame, emit the CSR entries (or, PACK, the kept packed words) ----
// acc (LDS, zeroed) += the block rows of the level-d voxel (ix, iy, iz) in its neighbour cells; cme: the neighbour cell of lane < 27,
// act: the lanes whose cell holds sites.  Cells are added in ascending stencil slot from 0 (k_row_diag repeats that order).
template <int NQ>
__device__ __forceinline__ void row_gather(const AsmArgs& A, int d, int ix, int iy, int iz, int lane, int cme, unsigned long long act, float* acc) {
    const int T = (A.hier.depth - d) * 27;
    // per-lane entry decomposition (independent of the neighbour cell)
    int edd[NQ], esx[NQ], esy[NQ], esz[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {      // lane l holds the NQ consecutive block columns NQ l .. NQ l + NQ - 1 (one vector load)
        const int t = NQ * lane + q, s = t % 27;
        edd[q] = t / 27;
        esx[q] = s / 9 - 1; esy[q] = (s / 3) % 3 - 1; esz[q] = s % 3 - 1;
    }
    // neighbour cells in batches of RF_BATCH: the block rows of a batch are requested together, and the next
    // batch is requested before the current one is accumulated in LDS (ablation: the block-row loads are
    // 3.2 of this kernel's 5.7 ms and latency-, not pattern-bound; one row in flight was too few, all 27 too many)
    constexpr int RF_BATCH = 4;
    float vb[2][RF_BATCH][NQ];
    int sp[2][RF_BATCH];
    auto fetch = [&](int buf) {
#pragma unroll
        for (int u = 0; u < RF_BATCH; ++u) {
            sp[buf][u] = -1;
            if (act) {
                const int spc = __ffsll((long long)act) - 1;
                act &= act - 1;
                sp[buf][u] = spc;
                const int c = __builtin_amdgcn_readlane(cme, spc);
                load_cols<NQ>(A.blocks[d] + ((int64_t)c * 27 + (26 - spc)) * T, lane, T, vb[buf][u]);
            }
        }
    };
    auto accumulate = [&](int buf) {
#pragma unroll
        for (int u = 0; u < RF_BATCH; ++u) {
            const int spc = sp[buf][u];
            if (spc < 0) continue;
            const int cx = ix + spc / 9 - 1, cy = iy + (spc / 3) % 3 - 1, cz = iz + spc % 3 - 1;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (NQ * lane + q < T) {
                    const int dd = edd[q];
                    const int rx = ((cx >> dd) + esx[q]) - (ix >> dd) + 2, ry = ((cy >> dd) + esy[q]) - (iy >> dd) + 2,
                              rz = ((cz >> dd) + esz[q]) - (iz >> dd) + 2;
                    acc[dd * 125 + (rz * 5 + ry) * 5 + rx] += vb[buf][u][q];
                }
            }
        }
    };
    fetch(0);
    while (sp[0][0] >= 0) {
        fetch(1);
        accumulate(0);
        if (sp[1][0] < 0) break;
        fetch(0);
        accumulate(1);
    }
}

// the kept entries of the row as packed words; cm: the row's colmap (structure comes from the count pass: no hashing here)
__device__ __forceinline__ void emit_packed(const AsmArgs& A, const AsmPackOut& K, int row, int lane, int nslots, const int32_t* cm,
                                            const float* acc, const int32_t* __restrict__ samelow, const int32_t* __restrict__ mir_off) {
    const float di = 1.f / sqrtf(K.diag[row]);
    const int local = K.local[row];
    const int base = K.new_of_old[row] - local;               // first new row of this row's segment
    int lpos = K.own_off[row];
    int opos = lpos + samelow[row];
    int mpos = mir_off[row];
    const int l0 = lpos, o0 = opos, m0 = mpos;
    for (int t0 = 0; t0 < nslots; t0 += 64) {
        const int t = t0 + lane;
        const int cv = (t < nslots) ? cm[t] : -1;
        const bool up = cv >= 0, low = cv <= -2;
        bool keep = false;
        __half hv = __ushort_as_half(0);
        int ncol = 0;
        if (up | low) {
            const int col = up ? cv : -2 - cv;
            hv = cc_scaled(acc[t], di, 1.f / sqrtf(K.diag[col]));
            keep = cc_keep(hv, K.drop);
            ncol = K.new_of_old[col];
        }
        const bool ku = keep && up, kl = keep && low, km = ku && t >= 125;
        const unsigned long long mu = __ballot(ku), ml = __ballot(kl), mm = __ballot(km);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (keep) {
            K.own[ku ? opos + __popcll(mu & below) : lpos + __popcll(ml & below)] = cc_word(hv, (uint32_t)(ncol - base));
            if (km) K.mir[mpos + __popcll(mm & below)] = ((uint64_t)(uint32_t)ncol << 32) | (uint64_t)cc_word(hv, (uint32_t)local & 0xFFFFu);
        }
        opos += __popcll(mu);
        lpos += __popcll(ml);
        mpos += __popcll(mm);
    }
    if (lane == 0) {
        K.kept[row] = lpos - l0;
        K.kept[(int64_t)(A.M + 1) + row] = opos - o0;
        K.kept[2 * (int64_t)(A.M + 1) + row] = mpos - m0;
    }
}

// row = [cross-level mirrors (from finer rows)][same-level lower][own upper][diagonal].  Same-level lower and
// own upper entries go straight to their final CSR slot; only the cross-level upper entries have a
// mirrored copy, which goes to a list keyed by destination row, sorted afterwards
__device__ __forceinline__ void emit_csr(const AsmArgs& A, int row, int lane, int nslots, const int32_t* cm, const float* acc,
                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ indeg,
                                         const int32_t* __restrict__ samelow, const int32_t* __restrict__ mir_off,
                                         int32_t* __restrict__ cols_out, float* __restrict__ vals_out, float* __restrict__ diag_out,
                                         uint64_t* __restrict__ mir_keys, float* __restrict__ mir_vals) {
    int64_t lpos = (int64_t)rowptr[row] + indeg[row];
    int64_t opos = lpos + samelow[row];
    int64_t mpos = (int64_t)mir_off[row];
    for (int t0 = 0; t0 < nslots; t0 += 64) {
        const int t = t0 + lane;
        const int cv = (t < nslots) ? cm[t] : -1;
        const bool up = cv >= 0, low = cv <= -2, mir = up && t >= 125;
        const unsigned long long mu = __ballot(up), ml = __ballot(low), mm = __ballot(mir);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (up | low) {
            const float v = acc[t];
            const int64_t k = up ? opos + __popcll(mu & below) : lpos + __popcll(ml & below);
            const int64_t ph = csr_phys(k, A.col_format);
            cols_out[ph] = up ? cv : -2 - cv;
            vals_out[ph] = v;
            if (mir) {
                const int64_t m = mpos + __popcll(mm & below);
                mir_keys[m] = ((uint64_t)row << A.col_bits) | (uint64_t)cv;   // low bits = destination row
                mir_vals[m] = v;
            }
        }
        opos += __popcll(mu);
        lpos += __popcll(ml);
        mpos += __popcll(mm);
    }
    if (lane == 0) {
        const float dv = acc[62] + A.reg;  // slot (dd=0, rel=(2,2,2))
        const int64_t ph = csr_phys(opos, A.col_format);
        cols_out[ph] = row;
        vals_out[ph] = dv;
        diag_out[row] = dv;
    }
}

template <int NQ, bool PACK>
__global__ void __launch_bounds__(ASM_WAVES * 64) k_row_fill(AsmArgs A, const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ indeg, const int32_t* __restrict__ samelow,
                                                             const int32_t* __restrict__ mir_off,
                                                             int32_t* __restrict__ cols_out, float* __restrict__ vals_out,
                                                             float* __restrict__ diag_out, uint64_t* __restrict__ mir_keys,
                                                             float* __restrict__ mir_vals,
                                                             float* __restrict__ b_out, int row_begin, int row_end, AsmPackOut K) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = row_begin + blockIdx.x * ASM_WAVES + wave;
    if (row >= row_end) return;
    const nksr_hier_t& h = A.hier;
    const int d = row_level(h, row);
    const nksr_level_t& lv = h.lv[d];
    const int i = row - lv.offset;
    const int ix = lv.ijk[i * 3], iy = lv.ijk[i * 3 + 1], iz = lv.ijk[i * 3 + 2];
    const int nslots = (h.depth - d) * 125;
    float* acc = lds + wave * (NKSR_MAX_DEPTH * 125);
    for (int t = lane; t < nslots; t += 64) acc[t] = 0.f;

    // neighbour cells and their site counts, one per lane
    const int cme = (lane < 27) ? lv.nbr[(int64_t)i * 27 + lane] : -1;
    const int nse = (cme >= 0) ? A.nsites[d][cme] : 0;
    if (!PACK) {                       // (the preconditioner's block has no right-hand side)
        float bl = (nse > 0) ? A.bvec[d][(int64_t)cme * 27 + (26 - lane)] : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bl += __shfl_xor(bl, o);
        if (lane == 0) b_out[row] = bl;
    }
    row_gather<NQ>(A, d, ix, iy, iz, lane, cme, __ballot(nse > 0), acc);
    const int32_t* cm = A.colmap[d] + (int64_t)i * nslots;
    if (PACK) emit_packed(A, K, row, lane, nslots, cm, acc, samelow, mir_off);
    else emit_csr(A, row, lane, nslots, cm, acc, rowptr, indeg, samelow, mir_off, cols_out, vals_out, diag_out, mir_keys, mir_vals);
}

// mirrored entries, stably sorted by destination row (sources ascending): final CSR slot
__global__ void k_place_mirrors(const uint64_t* __restrict__ keys, const float* __restrict__ vals, int64_t n, int col_bits,
                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ mirptr,
                                int32_t* __restrict__ cols_out, float* __restrict__ vals_out, int fmt) {
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const uint64_t key = keys[m];
    const int r = (int)(key & (((uint64_t)1 << col_bits) - 1));
    const int src = (int)(key >> col_bits);
    const int64_t ph = csr_phys((int64_t)rowptr[r] + (m - (int64_t)mirptr[r]), fmt);
    cols_out[ph] = src;
    vals_out[ph] = vals[m];
}

static int fill_args(AsmArgs& A, const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, float reg, int col_bits,
                     void* workspace) {
    if (h->depth < 1 || h->depth > NKSR_MAX_DEPTH) return nksr_set_error(NKSR_ERR_ARG, "bad depth %d", h->depth);
    if (nsets < 0 || nsets > 3) return nksr_set_error(NKSR_ERR_ARG, "at most 3 site sets");
    memset(&A, 0, sizeof(A));
    A.hier = *h;
    for (int s = 0; s < nsets; ++s) {
        if (!(sets[s].weight >= 0.f)) return nksr_set_error(NKSR_ERR_ARG, "site-set weights must be >= 0 (set %d: %g)", s, (double)sets[s].weight);
        A.sets[s] = sets[s];
    }
    A.nsets = nsets;
    A.M = h->lv[h->depth - 1].offset + h->lv[h->depth - 1].n;
    A.col_bits = col_bits;
    A.reg = reg;
    if (col_bits < 1 || col_bits > 32 || ((int64_t)1 << col_bits) < A.M) return nksr_set_error(NKSR_ERR_ARG, "col_bits too small");
    char* p = (char*)workspace;
    for (int d = 0; d < h->depth; ++d) {
        const AsmCarve s = asm_carve(h, d);
        A.blocks[d] = (float*)p; p += s.blocks;
        A.bvec[d] = (float*)p; p += s.bvec;
        A.nsites[d] = (int32_t*)p; p += s.nsites;
        A.colmap[d] = (int32_t*)p; p += s.colmap;
    }
    return NKSR_OK;
}

extern "C" size_t nksr_assemble_workspace_bytes(const nksr_hier_t* h) {
    size_t tot = 256;
    for (int d = 0; d < h->depth; ++d) {
        const AsmCarve s = asm_carve(h, d);
        tot += s.blocks + s.bvec + s.nsites + s.colmap;
    }
    return tot;
}

extern "C" int nksr_assemble_count(const nksr_hier_t* h, void* workspace, int32_t* rowcount, int32_t* crosscount, int32_t* samelow,
                                   int32_t* indeg, void* stream) {
    AsmArgs A;
    int M = h->lv[h->depth - 1].offset + h->lv[h->depth - 1].n;
    int cb = 1;
    while (((int64_t)1 << cb) < M) ++cb;
    int rc = fill_args(A, h, nullptr, 0, 0.f, cb, workspace);
    if (rc) return rc;
    if (A.M <= 0) return NKSR_OK;
    hipLaunchKernelGGL(k_row_count, dim3(nksr_blocks(A.M, ASM_WAVES * RC_RUN)), dim3(ASM_WAVES * 64), 0, (hipStream_t)stream, A, rowcount,
                       crosscount, samelow, indeg);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// phase 2b of every level.  K == nullptr: the CSR; otherwise the kept packed words (k_row_fill<.., true>)
static int launch_row_fill(const AsmArgs& A, const nksr_hier_t* h, const int32_t* rowptr, const int32_t* indeg, const int32_t* samelow,
                           const int32_t* mir_off, int32_t* cols_out, float* vals_out, float* diag_out, uint64_t* mir_keys,
                           float* mir_vals, float* b_out, const AsmPackOut* K, hipStream_t st) {
    const dim3 blk(ASM_WAVES * 64);
    const size_t lds = (size_t)ASM_WAVES * NKSR_MAX_DEPTH * 125 * sizeof(float);
    AsmPackOut none;
    memset(&none, 0, sizeof(none));
    for (int d = 0; d < h->depth; ++d) {
        const int n = h->lv[d].n;
        if (n <= 0) continue;
        const int T = (h->depth - d) * 27;
        const int r0 = h->lv[d].offset, r1 = r0 + n;
        const dim3 grid(nksr_blocks(n, ASM_WAVES));
        asm_with_width<3>(T > 128 ? 3 : (T > 64 ? 2 : 1), [&](auto nq) {      // floats per lane and block row (load_cols)
            constexpr int NQ = decltype(nq)::value;
            if (K) hipLaunchKernelGGL((k_row_fill<NQ, true>), grid, blk, lds, st, A, rowptr, indeg, samelow, mir_off, cols_out, vals_out,
                                      diag_out, mir_keys, mir_vals, b_out, r0, r1, *K);
            else hipLaunchKernelGGL((k_row_fill<NQ, false>), grid, blk, lds, st, A, rowptr, indeg, samelow, mir_off, cols_out, vals_out,
                                    diag_out, mir_keys, mir_vals, b_out, r0, r1, none);
        });
        NKSR_CHECK_LAUNCH();
    }
    return NKSR_OK;
}

extern "C" int nksr_assemble(const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, float reg, int col_bits,
                             void* workspace, const int32_t* rowptr, const int32_t* indeg, const int32_t* samelow,
                             const int32_t* mir_off, int col_format,
                             int32_t* cols_out, float* vals_out, float* diag_out, uint64_t* mir_keys, float* mir_vals,
                             float* b_out, void* split_scratch, size_t split_scratch_bytes, void* stream) {
    AsmArgs A;
    int rc = fill_args(A, h, sets, nsets, reg, col_bits, workspace);
    if (rc) return rc;
    if (col_format < 0 || col_format > 2) return nksr_set_error(NKSR_ERR_ARG, "col_format must be 0, 1 or 2");
    A.col_format = col_format;
    if (A.M <= 0) return NKSR_OK;
    rc = launch_cell_blocks(A, h, sets, nsets, split_scratch, split_scratch_bytes, (hipStream_t)stream);
    if (rc) return rc;
    return launch_row_fill(A, h, rowptr, indeg, samelow, mir_off, cols_out, vals_out, diag_out, mir_keys, mir_vals, b_out, nullptr,
                           (hipStream_t)stream);
}

extern "C" int nksr_assemble_packed(const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, float reg, void* workspace,
                                    const int32_t* samelow, const int32_t* mir_off, const int32_t* own_off, const int32_t* new_of_old,
                                    const int32_t* local_col, float drop_tol, float* diag_out, uint32_t* own_out, uint64_t* mir_out,
                                    int32_t* kept_out, void* split_scratch, size_t split_scratch_bytes, void* stream) {
    AsmArgs A;
    int rc = fill_args(A, h, sets, nsets, reg, 32, workspace);
    if (rc) return rc;
    if (!samelow || !mir_off || !own_off || !new_of_old || !local_col || !diag_out || !own_out || !mir_out || !kept_out)
        return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    if (!(drop_tol >= 0.f) || drop_tol >= 1.f) return nksr_set_error(NKSR_ERR_ARG, "drop_tol must be in [0, 1)");
    A.col_format = 2;
    if (A.M <= 0) return NKSR_OK;
    hipStream_t st = (hipStream_t)stream;
    rc = launch_cell_blocks(A, h, sets, nsets, split_scratch, split_scratch_bytes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_row_diag, dim3(nksr_blocks((int64_t)A.M * 32, 256)), dim3(256), 0, st, A, diag_out);
    NKSR_CHECK_LAUNCH();
    AsmPackOut K;
    K.diag = diag_out; K.new_of_old = new_of_old; K.local = local_col; K.own_off = own_off;
    K.own = own_out; K.mir = mir_out; K.kept = kept_out; K.drop = drop_tol;
    return launch_row_fill(A, h, nullptr, nullptr, samelow, mir_off, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &K, st);
}

extern "C" int nksr_place_mirrors(const uint64_t* keys_sorted, const float* vals_sorted, int64_t n, int col_bits,
                                  const int32_t* rowptr, const int32_t* mirptr, int col_format, int32_t* cols_out, float* vals_out,
                                  void* stream) {
    if (n <= 0) return NKSR_OK;
    if (col_format < 0 || col_format > 2) return nksr_set_error(NKSR_ERR_ARG, "col_format must be 0, 1 or 2");
    hipLaunchKernelGGL(k_place_mirrors, dim3(nksr_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, keys_sorted, vals_sorted, n,
                       col_bits, rowptr, mirptr, cols_out, vals_out, col_format);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
