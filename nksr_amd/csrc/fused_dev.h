// What the three parts of the matrix-free operator share: the geometry of the sweep, the arguments every
// kernel takes, the workspace they write into and the tests on finished segments.  csrc/fused_tables.hip builds the tables once
// per solve, csrc/fused_sweep.hip is the pass over the kernel rows (k_fz_cells), csrc/fused.hip the second product (k_fz_cellsum,
// k_fz_gather), the entry points and the solve.  Internal to the library: the symbols stay out of its dynamic table.
// (Not in common.h: build.kernel_hash('spmv') covers that file.)
#pragma once
#include "common.h"

// The row list is cut into ITEMS: item i = the units (see fused_tables.hip) that start in the 32-row window [32 i, 32 i + 32).  One
// item per 32-lane half of a wavefront (lane = stencil slot, 27 active), eight items per workgroup, up to four rows of a unit per trip.
#define FZ_RC 32
#define FZ_BLOCK 256
#define FZ_HW (FZ_BLOCK / 32)              // items (half-waves) of a workgroup
#define FZ_WG_ROWS (FZ_RC * FZ_HW)         // 256 consecutive rows per workgroup
#define FZ_TRIP 4                          // rows per trip (a normal site of the factor form -- header + three gradient rows -- is one trip)
#define FZ_GI 4                            // cells a half-wave of k_fz_cellsum takes at once

struct FusedArgs {               // uniform scalars and base pointers only
    const float* rows_all;       // [depth][rows_total][27]
    const float* targets_all;    // [rows_total]
    const int32_t* row_cells;    // [depth][rows_total]
    const int32_t* nbr32;        // [M][32]
    const int32_t* nbrT;         // [27][M]
    const int32_t* item_begin;   // [8 nwg + 1] first row of every item
    const int32_t* offsets;      // [M + 1] partial blocks of a cell
    const int32_t* multi;        // cells with partial blocks: the n_big cells that a whole workgroup of k_fz_cellsum sums first (the split,
                                 // at 16 blocks, is made by operator_tables in fields/operator_setup.py)
    int n_multi, n_big, M, depth;
    int hw_total;                // items (32-row windows of the row list)
    int64_t rows_total, nblocks;
    unsigned long long* nnz_counter;   // the set-up pass (MODE 1) leaves the non-zero slots of workgroup w in word 1 + w (plain stores:
                                       // no shared word); k_fz_count_sum adds them into word 0 (may be NULL)
    const int32_t* item_seg;     // [hw_total] segment of every 32-row item, [M] segment of every unknown (batched chunks; may be NULL)
    const int32_t* unknown_seg;
    const int* seg_done;         // device flags of the PCG: segment c finished <=> seg_done[c * seg_stride] != 0 (may be NULL)
    int seg_stride;
    const int* seg_done_count;   // device: finished segments so far (may be NULL); the per-cell sums and the gather look at their
    int seg_gate;                // unknowns' segments only once >= seg_gate have finished (the look-up costs ~20 % of those passes)
    // factor form (kernel_dim 4, see k_kernel_factors in kfield.hip): the rows are rebuilt in registers from 16-byte records
    const float4* fac_vec;       // [depth][rows_total] phi (position / header rows) or J_a (gradient rows), times sqrt(w); NULL = dense rows
    const float4* fac_pos;       // [rows_total] p = x * inv_w0 (3 floats) + the row's kind (int bits)
    const float4* psi_all;       // [M] psi of every unknown (levels concatenated)
    float inv_w0;
    int dense_from;              // set-up pass: the rebuilt rows of the levels >= dense_from are also written out dense
    float* dense_out;            // [depth - dense_from][rows_total][27] or NULL (the coarse-level block of the preconditioner reads them)
};

// workspace: [nblocks][32] partial blocks (x 2: the set-up pass makes two) + the set-up pass's second slot-major array [27][M]
struct FusedWork { float* part; float* part2; float* ct; float* ct2; };

static inline int fz_items(int64_t rows_total) { return (int)((rows_total + FZ_RC - 1) / FZ_RC); }
static inline int fz_nwg(int64_t rows_total) { return (fz_items(rows_total) + FZ_HW - 1) / FZ_HW; }

// ---- finished segments (batched chunks): their rows and unknowns are skipped, their y is never read again
__device__ __forceinline__ bool fz_seg_done(const FusedArgs& A, const int32_t* seg_of, int64_t i) {
    return A.seg_done && seg_of && A.seg_done[(int64_t)seg_of[i] * A.seg_stride] != 0;
}
__device__ __forceinline__ bool fz_gate_open(const FusedArgs& A) {
    return A.seg_done && A.unknown_seg && A.seg_done_count && *A.seg_done_count >= A.seg_gate;
}
// the segment of unknown j has finished (asked behind an open gate only)
__device__ __forceinline__ bool fz_unknown_done(const FusedArgs& A, int64_t j) {
    return A.seg_done[(int64_t)A.unknown_seg[j] * A.seg_stride] != 0;
}

#pragma GCC visibility push(hidden)
// the pass over the rows (csrc/fused_sweep.hip).  MODE 0: t from x, blocks into w.part / w.ct;  MODE 1: the set-up pass
template <int MODE>
void fz_sweep(const FusedArgs& A, const float* x, const FusedWork& w, const int* done, hipStream_t st);
#pragma GCC visibility pop
