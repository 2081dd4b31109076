// Phase 1 of the assembly (phases 2 to 4: csrc/assemble.hip): the per-cell Gram blocks on the fp32 matrix cores.
//
// All sites (input points / normal samples) inside one level-d cell c share their 27-voxel stencil at every level >= d, so their joint
// contribution is one dense block  B[d][c] = sum_sets w (R_d)^T [R_d .. R_{L-1} | t]  of shape 27 x (T + 1), T = 27 (L - d): a
// (27 x K)(K x (T + 1)) product, K = site rows of the cell.  Sites are Morton-sorted => contiguous per cell.  One wavefront per cell:
// v_mfma_f32_32x32x2_f32 with M = 27 (of 32) block rows, NT = ceil((T+1)/32) column tiles and
// two site rows per instruction (lanes 0-31 feed row 2m, lanes 32-63 row 2m+1; lane l supplies
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]).  Column T carries the right-hand side
// (27 m is never a multiple of 32, so a spare column always exists).  The set weight scales the A
// operand (the host passes rows pre-multiplied by sqrt(w) and weight 1, see below).  Accumulator register r of lane l is D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31].
// Every site row is read once per level (instead of once per touching matrix row: 27x less traffic than a direct gather).
// That column map is the site sets' (gram_rows, k_cell_blocks).  The operator's row list (asm_accumulate_lm) lets tile n hold
// LEVEL d + n instead, so that a half-wave load is one 108-byte row of one level's array: see asm_lm_pointers.
#include "assemble_dev.h"

typedef float asm_f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
__device__ __forceinline__ void asm_zero(asm_f32x16 (&acc)[NT]) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
}

// sites / site rows of cell c (row numbering inside a cell: set 0's rows, then set 1's)
__device__ __forceinline__ int asm_cell_sites(const AsmArgs& A, int d, int c) {
    int total = 0;
    for (int si = 0; si < A.nsets; ++si) total += A.sets[si].end[d][c] - A.sets[si].start[d][c];
    return total;
}
__device__ __forceinline__ int asm_cell_rows(const AsmArgs& A, int d, int c) {
    int R = 0;
    for (int si = 0; si < A.nsets; ++si) R += (A.sets[si].end[d][c] - A.sets[si].start[d][c]) * A.sets[si].ncomp;
    return R;
}

// entry `col` (slot col % 27 of level d + col / 27) of site row q: site-major rows [n ncomp, L, 27], or -- level_stride > 0 -- the
// level-major rows of the matrix-free operator ([L, level_stride, 27], site i at row row_index[i])
__device__ __forceinline__ float asm_row_value(const nksr_siteset_t& S, int64_t q, int L, int d, int col) {
    if (!S.level_stride) return S.val[(q * L + d) * 27 + col];
    const int dd = col / 27, s = col - dd * 27;
    const int64_t site = S.ncomp == 1 ? q : q / 3;
    const int64_t row = (S.row_index ? (int64_t)S.row_index[site] : site * S.ncomp) + (q - site * S.ncomp);
    return S.val[((int64_t)(d + dd - S.level_base) * S.level_stride + row) * 27 + s];
}

// writes the accumulated tile(s) of cell c: block rows whose voxel exists, the right-hand-side column, the site count
// ``by_level``: the accumulator tiles came from asm_accumulate_lm, whose tile n holds level d + n (slot j in lane j < 27, the
// right-hand side in lane 27 of tile 0) -- not columns 32 n .. 32 n + 31 of the concatenated levels
template <int NT>
__device__ __forceinline__ void cell_blocks_finalize(const AsmArgs& A, int d, int c, int lane, asm_f32x16 (&acc)[NT], int total, bool by_level = false) {
    const nksr_level_t& lv = A.hier.lv[d];
    const int T = (A.hier.depth - d) * 27;
    const int j = lane & 31, half = lane >> 5;
    if (lane == 0) A.nsites[d][c] = total;
    if (total == 0) return;
    float* out = A.blocks[d] + (int64_t)c * 27 * T;
    float* bv = A.bvec[d] + (int64_t)c * 27;
    // block row s is consumed by exactly one matrix row, the voxel at stencil slot s of this cell: rows whose
    // voxel does not exist are never read, so they are not written (about a third of the block traffic)
    const int nb = (lane < 27) ? lv.nbr[(int64_t)c * 27 + lane] : -1;
    const unsigned long long need = __ballot(nb >= 0);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = 32 * n + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int s = (r & 3) + 8 * (r >> 2) + 4 * half;
            if (s < 27 && ((need >> s) & 1ull)) {
                if (by_level) {
                    if (j < 27) { if (27 * n < T) out[s * T + 27 * n + j] = acc[n][r]; }
                    else if (n == 0 && j == 27) bv[s] = acc[n][r];
                } else {
                    if (col < T) out[s * T + col] = acc[n][r];
                    else if (col == T) bv[s] = acc[n][r];
                }
            }
        }
    }
}

// A coarse cell holds thousands of site rows (8x more per level): with one wavefront per cell the two coarsest levels of a
// tree_depth-5 chunk took 2.6 ms on ~8 k wavefronts.  The rows of such a cell are cut into PARTS -- a decision that depends on the
// cell alone: on a level that splits (asm_level_parts(d) > 1) a cell of R rows has min(level parts, R / ASM_PART_ROWS) parts of
// equal (even) length -- and its block is  sum over the parts, in order, of the part's own accumulator.  Two schedules give
// that same sum bit for bit: k_cell_blocks_part + k_cell_blocks_reduce (one wavefront per (cell, part), raw accumulator tiles
// through scratch; used when the level has few cells) and k_cell_blocks_seq (one wavefront per cell walks its parts; used when
// the level has enough cells to fill the chip, e.g. all chunks of a rank batched into one system).  The result therefore does
// not depend on how many other cells share the launch (tests/test_gpu_coarse_direct.py runs both schedules on the same cells).
#define ASM_PART_ROWS 128
#define ASM_TRIP 4
__host__ __device__ __forceinline__ int asm_level_parts(int d) {          // d = 0..2: 1, 3: 4, 4: 16, 5: 64
    const int k = d >= 2 ? (1 << (2 * (d - 2))) : 1;
    return k > 64 ? 64 : k;
}
// rows [lo, hi) of part p of a cell with R rows
__device__ __forceinline__ void asm_part_range(int R, int level_parts, int p, int& lo, int& hi) {
    int np = R / ASM_PART_ROWS;
    np = np < 1 ? 1 : (np > level_parts ? level_parts : np);
    const int rpp = ((R + np - 1) / np + 1) & ~1;                        // rows per part, even (two rows per MFMA)
    lo = p * rpp;
    hi = (p + 1) * rpp < R ? (p + 1) * rpp : R;
    if (lo > R) lo = R;
    if (hi < lo) hi = lo;
}

// ---- loop 1: the operator's row list --------------------------------------------------------------------------------------------
// The list as ONE site set (level-major rows, one row per "site", no row index: nksr_amd/fields/kernel_field.py
// assemble(fused_op=...)): rows [r_lo, r_hi) of the list, same products in the same order as gram_rows.  Every load is
// unconditional (clamped row, one pointer and one stride per lane and tile: the value of its column, or -- the lane of column T --
// the target), and the loads of the NEXT trip are requested before the products of this one: the pass ran at the latency of one
// trip after the other (~20 loads in flight per XCD against 200+ in the operator's sweep).
__device__ __forceinline__ bool asm_is_row_list(const AsmArgs& A) {
    return A.nsets == 1 && A.sets[0].level_stride > 0 && A.sets[0].ncomp == 1 && !A.sets[0].row_index;
}
template <int NT>
struct AsmLanePtr { const float* p[NT]; int mul[NT]; bool on[NT]; };
template <int NT>
__device__ __forceinline__ void asm_lm_load(const AsmLanePtr<NT>& P, int r0, int r_lo, int r_hi, int half, float (&b)[ASM_TRIP][NT]) {
#pragma unroll
    for (int u = 0; u < ASM_TRIP; ++u) {
        const int r = r0 + 2 * u + half;
        const int rc = r < r_hi ? r : r_lo;
#pragma unroll
        for (int n = 0; n < NT; ++n) b[u][n] = P.p[n][(int64_t)rc * P.mul[n]];
    }
}
template <int NT>
__device__ __forceinline__ void asm_lm_mfma(const AsmLanePtr<NT>& P, int r0, int r_hi, int half, int j, float w, float (&b)[ASM_TRIP][NT], asm_f32x16 (&acc)[NT]) {
#pragma unroll
    for (int u = 0; u < ASM_TRIP; ++u) {
        const bool ok = r0 + 2 * u + half < r_hi;
        float v[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) v[n] = (ok && P.on[n]) ? b[u][n] : 0.f;
        const float a = (j < 27) ? w * v[0] : 0.f;
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v[n], acc[n], 0, 0, 0);
    }
}
// lane pointers of level d's column tiles (they do not depend on the cell).  Tile n holds LEVEL d + n: slot j in lane j < 27 (NT =
// ceil((T + 1) / 32) tiles are as many as there are levels, because 27 <= 32), the right-hand side in lane 27 of tile 0; the lanes
// left over are clamped onto slot 26 of their tile's row and masked.  A half-wave load is then ONE 108-byte row of one level's array
// (with columns 32 n + j it straddled two levels' arrays, which lie level_stride rows apart, and the idle lanes of the last tile read
// a third place: 4-6 cache lines per load instruction for two rows where 2-4 do).  Every block element is still the sum of the same
// products over the rows in the same order -- only the (tile, lane) that holds it moved, cell_blocks_finalize(by_level) knows where.
template <int NT>
__device__ __forceinline__ void asm_lm_pointers(const AsmArgs& A, int d, int lane, AsmLanePtr<NT>& P) {
    const nksr_siteset_t& S = A.sets[0];
    const int levels = A.hier.depth - d;
    const int j = lane & 31;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const bool rhs = n == 0 && j == 27 && S.target;
        const int dd = n < levels ? n : 0;      // (a tile past the last level is never used but its loads are unconditional: it reads level d)
        P.on[n] = (n < levels && j < 27) || rhs;
        P.mul[n] = rhs ? 1 : 27;
        P.p[n] = rhs ? S.target : S.val + (int64_t)(d + dd - S.level_base) * S.level_stride * 27 + (j < 27 ? j : 26);
    }
}
template <int NT>
__device__ __forceinline__ void asm_accumulate_lm(const AsmArgs& A, int d, int r_lo, int r_hi, int lane, asm_f32x16 (&acc)[NT]) {
    if (r_hi <= r_lo) return;
    const nksr_siteset_t& S = A.sets[0];
    const int j = lane & 31, half = lane >> 5;
    AsmLanePtr<NT> P;
    asm_lm_pointers<NT>(A, d, lane, P);
    const float w = S.weight;
    float bA[ASM_TRIP][NT], bB[ASM_TRIP][NT];
    asm_lm_load<NT>(P, r_lo, r_lo, r_hi, half, bA);
    for (int r0 = r_lo; r0 < r_hi; r0 += 4 * ASM_TRIP) {
        const int r1 = r0 + 2 * ASM_TRIP, r2 = r0 + 4 * ASM_TRIP;
        if (r1 < r_hi) asm_lm_load<NT>(P, r1, r_lo, r_hi, half, bB);
        asm_lm_mfma<NT>(P, r0, r_hi, half, j, w, bA, acc);
        if (r1 < r_hi) {
            if (r2 < r_hi) asm_lm_load<NT>(P, r2, r_lo, r_hi, half, bA);
            asm_lm_mfma<NT>(P, r1, r_hi, half, j, w, bB, acc);
        }
    }
}

// ---- loop 2: site sets, either row layout, any range of a cell's rows ---------------------------------------------------------------
// acc += the Gram products of rows [lo, hi) of cell c (row numbering: set 0's rows, then set 1's).
// ASM_TRIP row pairs per trip: their loads go out together, every one of them unconditional on a clamped row (one pair per trip left
// the wavefront waiting on every load; the pass is bound by the loads in flight -- 20 per XCD at four pairs, against 200+ in the
// operator's sweep).  For cells of 60+ rows: the coarse block of the preconditioner, and the levels that split.
template <int NT>
__device__ __forceinline__ void gram_rows(const AsmArgs& A, int d, int c, int lo, int hi, int lane, asm_f32x16 (&acc)[NT]) {
    const int L = A.hier.depth;
    const int T = (L - d) * 27;
    const int j = lane & 31, half = lane >> 5;
    int base = 0;
    for (int si = 0; si < A.nsets; ++si) {
        const nksr_siteset_t& S = A.sets[si];
        const int k0 = S.start[d][c], k1 = S.end[d][c];
        const int nrows = (k1 - k0) * S.ncomp;
        const int m_lo = lo > base ? lo - base : 0, m_hi = hi - base < nrows ? hi - base : nrows;      // this set's rows of the range
        const int64_t q0 = (int64_t)k0 * S.ncomp;
        const float w = S.weight;
        for (int m0 = m_lo; m0 < m_hi; m0 += 2 * ASM_TRIP) {
            float b[ASM_TRIP][NT];
#pragma unroll
            for (int u = 0; u < ASM_TRIP; ++u) {
                const int m = m0 + 2 * u + half;
                const bool valid = m < m_hi;
                const int64_t q = q0 + (valid ? m : m_lo);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int col = 32 * n + j;
                    float v = 0.f;
                    if (col < T) v = asm_row_value(S, q, L, d, col);
                    else if (col == T && S.target) v = S.target[q];
                    b[u][n] = valid ? v : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < ASM_TRIP; ++u) {
                const float a = (j < 27) ? w * b[u][0] : 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[u][n], acc[n], 0, 0, 0);
            }
        }
        base += nrows;
    }
}

// acc += the Gram products of rows [lo, hi) of cell c (hi: at most the cell's rows), from the row list or from the site sets
template <int NT>
__device__ __forceinline__ void gram_accumulate(const AsmArgs& A, int d, int c, int lo, int hi, int lane, asm_f32x16 (&acc)[NT]) {
    if (asm_is_row_list(A)) asm_accumulate_lm<NT>(A, d, A.sets[0].start[d][c] + lo, A.sets[0].start[d][c] + hi, lane, acc);
    else gram_rows<NT>(A, d, c, lo, hi, lane, acc);
}

// ---- the kernels: which cell, which range(s), accumulate, finalize or store ----------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(ASM_WAVES * 64) k_cell_blocks_part(AsmArgs A, int d, int nsplit, float* __restrict__ scratch) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const nksr_level_t& lv = A.hier.lv[d];
    const int64_t idx = (int64_t)blockIdx.x * ASM_WAVES + wave;
    if (idx >= (int64_t)lv.n * nsplit) return;
    const int c = (int)(idx / nsplit), p = (int)(idx - (int64_t)c * nsplit);
    asm_f32x16 acc[NT];
    asm_zero(acc);
    int lo, hi;
    asm_part_range(asm_cell_rows(A, d, c), nsplit, p, lo, hi);
    gram_accumulate<NT>(A, d, c, lo, hi, lane, acc);
    float* out = scratch + idx * (NT * 16 * 64) + lane;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(n * 16 + r) * 64] = acc[n][r];
}

template <int NT>
__global__ void __launch_bounds__(ASM_WAVES * 64) k_cell_blocks_reduce(AsmArgs A, int d, int nsplit, const float* __restrict__ scratch) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * ASM_WAVES + wave;
    if (c >= A.hier.lv[d].n) return;
    asm_f32x16 acc[NT];
    asm_zero(acc);
    for (int p = 0; p < nsplit; ++p) {
        const float* in = scratch + ((int64_t)c * nsplit + p) * (NT * 16 * 64) + lane;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[n][r] += in[(n * 16 + r) * 64];
    }
    cell_blocks_finalize<NT>(A, d, c, lane, acc, asm_cell_sites(A, d, c), asm_is_row_list(A));
}

// the same sum, one wavefront per cell: part after part into a fresh accumulator, added to the total in order
template <int NT>
__global__ void __launch_bounds__(ASM_WAVES * 64) k_cell_blocks_seq(AsmArgs A, int d, int nsplit) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * ASM_WAVES + wave;
    if (c >= A.hier.lv[d].n) return;
    asm_f32x16 tot[NT];
    asm_zero(tot);
    const int R = asm_cell_rows(A, d, c);
    for (int p = 0; p < nsplit; ++p) {
        int lo, hi;
        asm_part_range(R, nsplit, p, lo, hi);
        asm_f32x16 acc[NT];
        asm_zero(acc);
        if (hi > lo) gram_accumulate<NT>(A, d, c, lo, hi, lane, acc);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[n][r] += acc[n][r];
    }
    cell_blocks_finalize<NT>(A, d, c, lane, tot, asm_cell_sites(A, d, c), asm_is_row_list(A));
}

// A level that does not split: the whole cell into one accumulator (not k_cell_blocks_seq with one part: 0.f + acc is not acc for
// -0, and a second accumulator costs registers).  LM: the site sets hold LEVEL-MAJOR rows (nksr_siteset_t.level_stride > 0)
template <int NT, bool LM>
__global__ void __launch_bounds__(ASM_WAVES * 64) k_cell_blocks(AsmArgs A, int d) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const nksr_level_t& lv = A.hier.lv[d];
    const int c = blockIdx.x * ASM_WAVES + wave;
    if (c >= lv.n) return;
    const int L = A.hier.depth;
    const int T = (L - d) * 27;
    const int j = lane & 31, half = lane >> 5;
    asm_f32x16 acc[NT];
    asm_zero(acc);
    if (LM) {
        gram_accumulate<NT>(A, d, c, 0, asm_cell_rows(A, d, c), lane, acc);
        cell_blocks_finalize<NT>(A, d, c, lane, acc, asm_cell_sites(A, d, c), asm_is_row_list(A));
        return;
    }
    // ---- loop 3: all rows of a cell of site-major sets (the assembled solve), one row pair per trip.  Fine cells hold ~3 rows;
    // batching the loads of two pairs (as gram_rows does) measured 25 % slower here.  It is no instance of gram_rows, and not even a
    // function of its own: in either form the compiler adds the lane's column offset to the row address on every trip (and, as
    // gram_rows with one pair per trip, forms the row address anew with three 64-bit multiply-adds) where this loop adds a stride.
    // The site count comes out of the same walk over the sets: a wavefront lives for ~3 rows, asm_cell_sites would be a second
    // chain of dependent loads.
    int total = 0;
    for (int si = 0; si < A.nsets; ++si) {
        const nksr_siteset_t& S = A.sets[si];
        const int k0 = S.start[d][c], k1 = S.end[d][c];
        if (k0 >= k1) continue;
        total += k1 - k0;
        const int64_t q0 = (int64_t)k0 * S.ncomp;
        const int nrows = (k1 - k0) * S.ncomp;
        // The set weight multiplies the A operand.  Callers that need BITWISE symmetric same-level blocks (the
        // row fill emits same-level lower entries from the row's own frame) pass rows and targets
        // pre-multiplied by sqrt(w) and weight 1 (nksr_amd/fields/kernel_field.py does): the products
        // (sw r_s)(sw r_t) then commute exactly.  Keep this loop as it is -- variants that dropped the multiply,
        // added a second code path (88 VGPRs) or called sqrtf here all measured 20 % slower.
        const float w = S.weight;
        for (int m0 = 0; m0 < nrows; m0 += 2) {
            const bool valid = m0 + half < nrows;
            const int64_t q = q0 + m0 + half;
            const float* ra = S.val + (q * L + d) * 27;
            float b[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int col = 32 * n + j;
                b[n] = 0.f;
                if (valid) {
                    if (col < T) b[n] = ra[col];
                    else if (col == T && S.target) b[n] = S.target[q];
                }
            }
            const float a = (j < 27) ? w * b[0] : 0.f;
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[n], acc[n], 0, 0, 0);
        }
    }
    cell_blocks_finalize<NT>(A, d, c, lane, acc, total);
}

// column tiles of level d, incl. the right-hand-side column
static int asm_tiles(const nksr_hier_t* h, int d) { return ((h->depth - d) * 27 + 32) / 32; }

// phase 1 of every level: the per-cell Gram blocks
int launch_cell_blocks(const AsmArgs& A, const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, void* split_scratch,
                       size_t split_scratch_bytes, hipStream_t st) {
    const dim3 blk(ASM_WAVES * 64);
    bool lm = false;
    for (int si = 0; si < nsets; ++si) {
        if (si > 0 && (sets[si].level_stride != 0) != lm) return nksr_set_error(NKSR_ERR_ARG, "site sets mix site-major and level-major rows");
        if (sets[si].level_base < 0 || sets[si].level_base >= h->depth || (sets[si].level_base > 0 && !sets[si].level_stride))
            return nksr_set_error(NKSR_ERR_ARG, "site set: level_base needs level-major rows and a level of the hierarchy");
        lm = sets[si].level_stride != 0;
        for (int d = 0; d < sets[si].level_base; ++d)
            if (h->lv[d].n > 0) return nksr_set_error(NKSR_ERR_ARG, "site set: rows start at level %d but level %d of the hierarchy has cells", (int)sets[si].level_base, d);
    }
    for (int d = 0; d < h->depth; ++d) {
        const int n = h->lv[d].n;
        if (n <= 0) continue;
        const int NT = asm_tiles(h, d);
        const dim3 grid(nksr_blocks(n, ASM_WAVES));
        // the part structure is a property of the level (and the cell); the schedule is picked by size -- same bits either way
        const int nsplit = asm_level_parts(d);
        const size_t need = asm_split_bytes(n, nsplit, (size_t)NT);
        const bool par = split_scratch && need && need <= split_scratch_bytes;
        asm_with_width<6>(NT, [&](auto nt) {
            constexpr int N = decltype(nt)::value;
            if (nsplit <= 1) {
                if (lm) hipLaunchKernelGGL((k_cell_blocks<N, true>), grid, blk, 0, st, A, d);
                else hipLaunchKernelGGL((k_cell_blocks<N, false>), grid, blk, 0, st, A, d);
            } else if (par) {
                hipLaunchKernelGGL((k_cell_blocks_part<N>), dim3(nksr_blocks((int64_t)n * nsplit, ASM_WAVES)), blk, 0, st, A, d, nsplit, (float*)split_scratch);
                hipLaunchKernelGGL((k_cell_blocks_reduce<N>), grid, blk, 0, st, A, d, nsplit, (const float*)split_scratch);
            } else {
                hipLaunchKernelGGL((k_cell_blocks_seq<N>), grid, blk, 0, st, A, d, nsplit);
            }
        });
        NKSR_CHECK_LAUNCH();
    }
    return NKSR_OK;
}

extern "C" size_t nksr_assemble_split_bytes(const nksr_hier_t* h) {
    size_t best = 0;
    for (int d = 0; d < h->depth; ++d) {
        const size_t b = asm_split_bytes(h->lv[d].n, asm_level_parts(d), (size_t)asm_tiles(h, d));
        if (b > best) best = b;
    }
    return best;
}
