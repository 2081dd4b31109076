// Matrix-free ("fused") normal-equation operator  y = (sum_s R_s^T R_s + reg I) x  and its Jacobi-PCG solve.
// Reference: reconstruct(..., fused_mode=True) (examples/recons_waymo.py:33, recons_waymo_cpu.py:58, gis_app.py:40) -- the
// memory-lean solve that never materialises the system matrix; KernelField.solve (the assembled twin is solve_non_fused,
// models/nksr_net.py:105-112).
//
// One application is three launches.  The sweep over the kernel rows (k_fz_cells, csrc/fused_sweep.hip) leaves, for every cell c,
// the block  P[c][s] = sum_{r in c} rows[r][s] t[r]:  slot-major in ct[s][c] when the rows of c lie inside one workgroup of the
// sweep, as one partial block per workgroup otherwise (the coarse cells, ~1 % of them).  This file holds the second product:
//   k_fz_cellsum  ct[s][c] = the partial blocks of c added in a fixed order (the cells of A.multi only)
//   k_fz_gather   y_j = reg x_j + sum_s' ct[26 - s'][nbrT[s'][j]], one lane per unknown: 27 coalesced loads of the slot-major
//                 neighbour table and 27 gathers whose 64 lanes hit a few neighbouring lines (consecutive unknowns have
//                 consecutive neighbours)
// and the host side: the workspace, the entry points and the operator the shared PCG driver (csrc/pcg.hip) iterates with.  The
// tables all three read are built once per solve (csrc/fused_tables.hip).  No float atomics, every order of summation fixed.
#include "fused_dev.h"
#include "pcg_core.h"
#include <stdlib.h>

// true when the FZ_GI (four) cells idx[i0 ..] of this half-wave all belong to finished segments (gated, see seg_gate).
// n: valid entries from i0 on.
__device__ __forceinline__ bool fz_group_done(const FusedArgs& A, const int32_t* idx, int64_t i0, int n, int lane32, bool upper) {
    if (!fz_gate_open(A)) return false;
    bool dn = true;
    if (lane32 < FZ_GI && lane32 < n) dn = fz_unknown_done(A, idx ? idx[i0 + lane32] : i0 + lane32);
    return (unsigned)(__ballot(dn) >> (upper ? 32 : 0)) == 0xFFFFFFFFu;
}

// ct[s][c] = sum of the partial blocks of cell c (one per workgroup of the sweep its rows reach into: the cells of A.multi --
// coarse cells, hundreds of blocks each; cells inside one workgroup never get here).  A half-wave takes FOUR cells at once
// (lane = slot): the pass is latency-bound, the first two blocks of the four cells are requested together.  Fixed order.
__global__ void __launch_bounds__(256) k_fz_cellsum(FusedArgs A, const float* __restrict__ part, float* __restrict__ ct,
                                                   const int* __restrict__ done) {
    if (done && *done) return;
    const int s = threadIdx.x & 31;
    if ((int)blockIdx.x < A.n_big) {
        // a coarse cell with many blocks (A.multi[0 .. n_big)): the whole workgroup sums it -- half-wave h takes blocks h, h + 8, ...
        // (one serial chain over hundreds of blocks was the critical path of the pass), then the eight partial sums in order
        __shared__ float partial[8][32];
        const int cell = A.multi[blockIdx.x], h = threadIdx.x >> 5;
        if (fz_gate_open(A) && fz_unknown_done(A, cell)) return;          // uniform over the workgroup
        const int b0 = A.offsets[cell], n = A.offsets[cell + 1] - b0;
        const float* p = part + (int64_t)(b0 + h) * 32 + s;
        float acc = 0.f;
        int b = h;
        // (sixteen blocks requested per trip, added in the order of the four-block trips they replace: a cell of hundreds of blocks was a
        // chain of as many dependent round trips / 4)
        for (; b + 120 < n; b += 128, p += 4096) {
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = p[256 * q];
#pragma unroll
            for (int q = 0; q < 16; q += 4) acc += (v[q] + v[q + 1]) + (v[q + 2] + v[q + 3]);
        }
        for (; b + 24 < n; b += 32, p += 1024) acc += (p[0] + p[256]) + (p[512] + p[768]);
        for (; b < n; b += 8, p += 256) acc += p[0];
        partial[h][s] = acc;
        __syncthreads();
        if (h == 0 && s < 27) {
            float t = partial[0][s];
#pragma unroll
            for (int k = 1; k < 8; ++k) t += partial[k][s];
            ct[(int64_t)s * A.M + cell] = t;
        }
        return;
    }
    const int first = A.n_big, ncell = A.n_multi - first;
    const int i0 = ((((int)blockIdx.x - A.n_big) * 256 + (int)threadIdx.x) >> 5) * FZ_GI;
    if (i0 >= ncell) return;
    if (fz_group_done(A, A.multi + first, i0, ncell - i0, s, (threadIdx.x & 32) != 0)) return;
    int cell[FZ_GI], b0[FZ_GI], n[FZ_GI];
#pragma unroll
    for (int k = 0; k < FZ_GI; ++k) cell[k] = A.multi[first + (i0 + k < ncell ? i0 + k : ncell - 1)];
#pragma unroll
    for (int k = 0; k < FZ_GI; ++k) {
        b0[k] = A.offsets[cell[k]];
        n[k] = i0 + k < ncell ? A.offsets[cell[k] + 1] - b0[k] : 0;
    }
    float acc[FZ_GI], a1[FZ_GI];
#pragma unroll
    for (int k = 0; k < FZ_GI; ++k) {
        acc[k] = n[k] > 0 ? part[(int64_t)b0[k] * 32 + s] : 0.f;
        a1[k] = n[k] > 1 ? part[(int64_t)(b0[k] + 1) * 32 + s] : 0.f;
    }
    // the four cells' chains side by side (each cell's own order of additions as before: four blocks per trip, then one by one)
    int nmax = 0;
#pragma unroll
    for (int k = 0; k < FZ_GI; ++k) { acc[k] += a1[k]; nmax = n[k] > nmax ? n[k] : nmax; }
    for (int b = 2; b < nmax; b += 4) {
        float v[FZ_GI][4];
#pragma unroll
        for (int k = 0; k < FZ_GI; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[k][q] = b + q < n[k] ? part[(int64_t)(b0[k] + b + q) * 32 + s] : 0.f;
#pragma unroll
        for (int k = 0; k < FZ_GI; ++k) {
            if (b + 4 <= n[k]) acc[k] += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (b + q < n[k]) acc[k] += v[k][q];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FZ_GI; ++k)
        if (i0 + k < ncell && s < 27) ct[(int64_t)s * A.M + cell[k]] = acc[k];
}

// y_j = (MODE 0: reg x_j, 1: 0, 2: reg) + sum over the 27 neighbour cells c = nbrT[s'][j] of j:  ct[26 - s'][c]
// One lane per unknown: the 27 table loads are coalesced, the 27 gathers of 64 consecutive unknowns hit a few neighbouring lines
// each (consecutive unknowns have consecutive neighbours).  Fixed summation tree.  Workgroups are dealt to the XCDs round-robin by
// the hardware: workgroup 8 i + k takes the i-th group of the k-th EIGHTH of the unknowns, so that an XCD's L2 holds one contiguous
// (Morton-ordered) part of ct instead of every XCD fetching all of it.
template <int MODE>
__global__ void __launch_bounds__(256) k_fz_gather(FusedArgs A, int per_xcd, const float* __restrict__ ct, const float* __restrict__ x,
                                                  float reg, float* __restrict__ y, const int* __restrict__ done) {
    if (done && *done) return;
    const int xcd = blockIdx.x & 7, grp = blockIdx.x >> 3;
    const int local = grp * 256 + threadIdx.x;
    if (local >= per_xcd) return;
    const int j = xcd * per_xcd + local;
    if (j >= A.M) return;
    if (fz_gate_open(A) && fz_unknown_done(A, j)) return;
    int c[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) c[k] = A.nbrT[(int64_t)k * A.M + j];
    float v[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) v[k] = ct[(int64_t)(26 - k) * A.M + (c[k] >= 0 ? c[k] : 0)];
#pragma unroll
    for (int k = 0; k < 27; ++k) v[k] = c[k] >= 0 ? v[k] : 0.f;
    // fixed tree: 27 -> 9 -> 3 -> 1
    float r9[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r9[k] = (v[3 * k] + v[3 * k + 1]) + v[3 * k + 2];
    const float r = ((r9[0] + r9[1]) + r9[2]) + ((r9[3] + r9[4]) + r9[5]) + ((r9[6] + r9[7]) + r9[8]);
    y[j] = r + (MODE == 0 ? reg * x[j] : (MODE == 2 ? reg : 0.f));
}
// nnz_counter[0] += the per-workgroup counts of the set-up sweep (integers: order-free; one add per FZ_CS_PER entries)
#define FZ_CS_PER 4096
__global__ void __launch_bounds__(256) k_fz_count_sum(unsigned long long* __restrict__ counter, int nwg) {
    __shared__ unsigned long long wsum[4];
    unsigned long long v = 0;
    const int i0 = blockIdx.x * FZ_CS_PER, i1 = i0 + FZ_CS_PER < nwg ? i0 + FZ_CS_PER : nwg;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) v += counter[1 + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(counter, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// ---- the second product's launches -------------------------------------------------------------------------------------------------
static void fz_cellsum(const FusedArgs& A, const float* part, float* ct, const int* done, hipStream_t st) {
    if (A.n_multi > 0)
        hipLaunchKernelGGL(k_fz_cellsum, dim3(A.n_big + nksr_blocks(((int64_t)(A.n_multi - A.n_big) + FZ_GI - 1) / FZ_GI * 32, 256)), dim3(256), 0, st, A,
                           part, ct, done);
}
template <int MODE>
static void fz_gather(const FusedArgs& A, const float* ct, const float* x, float reg, float* y, const int* done, hipStream_t st) {
    const int per_xcd = ((A.M + 7) / 8 + 255) / 256 * 256;           // an eighth of the unknowns, in whole workgroups
    hipLaunchKernelGGL((k_fz_gather<MODE>), dim3((unsigned)(per_xcd / 256 * 8)), dim3(256), 0, st, A, per_xcd, ct, x, reg, y, done);
}

static int fz_apply(const FusedArgs& A, float reg, const FusedWork& w, const float* x, float* y, const int* done, hipStream_t st) {
    fz_sweep<0>(A, x, w, done, st);
    fz_cellsum(A, w.part, w.ct, done, st);
    fz_gather<0>(A, w.ct, x, reg, y, done, st);
    return NKSR_OK;
}

// ---- workspace and arguments ---------------------------------------------------------------------------------------------------------
static size_t fz_align(size_t v) { return (v + 255) / 256 * 256; }
static size_t fz_blocks_bytes(int64_t nblocks) { return fz_align((size_t)(nblocks > 0 ? nblocks : 1) * 32 * sizeof(float)); }
extern "C" size_t nksr_fused_workspace_bytes(int64_t nblocks, int32_t M) {
    return 2 * fz_blocks_bytes(nblocks) + fz_align((size_t)(M > 0 ? M : 1) * 27 * sizeof(float));
}
static FusedWork fz_carve(const nksr_fused_op_t* op) {
    FusedWork w;
    w.part = (float*)op->workspace;
    w.part2 = (float*)((char*)op->workspace + fz_blocks_bytes(op->nblocks));
    w.ct2 = (float*)((char*)op->workspace + 2 * fz_blocks_bytes(op->nblocks));
    w.ct = op->cell_sums;
    return w;
}

static int fz_args(FusedArgs& A, const nksr_fused_op_t* op) {
    if (!op) return nksr_set_error(NKSR_ERR_ARG, "operator is NULL");
    if (op->depth < 1 || op->depth > NKSR_MAX_DEPTH) return nksr_set_error(NKSR_ERR_ARG, "bad depth %d", op->depth);
    const bool fac = op->fac_vec != nullptr;
    if (fac && (!op->fac_pos || !op->psi_all || !(op->inv_w0 > 0.f) || (((uintptr_t)op->fac_vec | (uintptr_t)op->fac_pos | (uintptr_t)op->psi_all) & 15)))
        return nksr_set_error(NKSR_ERR_ARG, "factor form: fac_pos / psi_all / inv_w0 missing or arrays not 16-byte aligned");
    if (op->dense_out && (!fac || op->dense_from < 0 || op->dense_from >= op->depth))
        return nksr_set_error(NKSR_ERR_ARG, "dense_out needs the factor form and 0 <= dense_from < depth");
    if (op->M > 0 && ((!op->rows_all && !fac) || !op->row_cells || !op->nbr32 || !op->nbrT || !op->item_begin || !op->offsets || !op->workspace || !op->cell_sums ||
                      (op->n_multi > 0 && !op->multi) || op->n_big < 0 || op->n_big > op->n_multi))
        return nksr_set_error(NKSR_ERR_ARG, "operator has NULL arrays");
    if (op->rows_total < 0 || op->rows_total >= ((int64_t)1 << 31) - 2 * FZ_WG_ROWS || op->nblocks >= ((int64_t)1 << 31) - ((int64_t)1 << 26))
        return nksr_set_error(NKSR_ERR_CAPACITY, "operator too large");
    memset(&A, 0, sizeof(A));
    A.rows_all = op->rows_all; A.targets_all = op->targets_all; A.row_cells = op->row_cells; A.nbr32 = op->nbr32; A.nbrT = op->nbrT; A.item_begin = op->item_begin; A.offsets = op->offsets;
    A.multi = op->multi; A.n_multi = op->n_multi; A.n_big = op->n_big;
    A.M = op->M; A.depth = op->depth; A.rows_total = op->rows_total; A.nblocks = op->nblocks;
    A.nnz_counter = (unsigned long long*)op->nnz_counter;
    A.item_seg = op->item_seg; A.unknown_seg = op->unknown_seg;
    A.hw_total = fz_items(op->rows_total);
    A.fac_vec = (const float4*)op->fac_vec; A.fac_pos = (const float4*)op->fac_pos; A.psi_all = (const float4*)op->psi_all;
    A.inv_w0 = op->inv_w0; A.dense_from = op->dense_from; A.dense_out = op->dense_out;
    return NKSR_OK;
}

// what the operator's entry points start with: the arguments checked, nothing to do for an empty system, the workspace carved.
// body(A, w) enqueues the work and returns a status
template <class F>
static int fz_with_op(const nksr_fused_op_t* op, F&& body) {
    FusedArgs A;
    if (int rc = fz_args(A, op)) return rc;
    if (A.M <= 0) return NKSR_OK;
    if (int rc = body(A, fz_carve(op))) return rc;
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int nksr_fused_apply(const nksr_fused_op_t* op, float reg, const float* x, float* y, void* stream) {
    return fz_with_op(op, [&](const FusedArgs& A, const FusedWork& w) { return fz_apply(A, reg, w, x, y, nullptr, (hipStream_t)stream); });
}

extern "C" int nksr_fused_rhs_diag(const nksr_fused_op_t* op, float reg, float* b_out, float* diag_out, void* stream) {
    return fz_with_op(op, [&](const FusedArgs& A, const FusedWork& w) -> int {
        hipStream_t st = (hipStream_t)stream;
        if (b_out && !A.targets_all) return nksr_set_error(NKSR_ERR_ARG, "targets_all is NULL");
        if (!b_out && !diag_out) return NKSR_OK;
        // one sweep over the rows makes the per-cell sums of both (and counts the stored entries); cells without rows keep their zeros
        if (A.nnz_counter) (void)hipMemsetAsync(A.nnz_counter, 0, sizeof(unsigned long long), st);
        NKSR_CHECK_HIP(hipMemsetAsync(w.ct2, 0, (size_t)A.M * 27 * sizeof(float), st));
        fz_sweep<1>(A, nullptr, w, nullptr, st);
        if (A.nnz_counter && A.hw_total > 0) {
            const int nwg = fz_nwg(A.rows_total);
            hipLaunchKernelGGL(k_fz_count_sum, dim3(nksr_blocks(nwg, FZ_CS_PER)), dim3(256), 0, st, A.nnz_counter, nwg);
        }
        // b from part / ct, the diagonal from part2 / ct2: the same two calls
        if (b_out) { fz_cellsum(A, w.part, w.ct, nullptr, st); fz_gather<1>(A, w.ct, nullptr, reg, b_out, nullptr, st); }
        if (diag_out) { fz_cellsum(A, w.part2, w.ct2, nullptr, st); fz_gather<2>(A, w.ct2, nullptr, reg, diag_out, nullptr, st); }
        return NKSR_OK;
    });
}

extern "C" int nksr_fused_expand_rows(const nksr_fused_op_t* op, void* stream) {
    return fz_with_op(op, [&](FusedArgs A, const FusedWork& w) -> int {
        if (!A.fac_vec || !A.dense_out) return nksr_set_error(NKSR_ERR_ARG, "expand_rows needs the factor form and dense_out");
        A.nnz_counter = nullptr;
        fz_sweep<1>(A, nullptr, w, nullptr, (hipStream_t)stream);
        return NKSR_OK;
    });
}

struct FusedOperator : PcgOperator {
    FusedArgs A; float reg; FusedWork w;
    int apply(const float* p, float* y, const int* done, const int* seg_done, int seg_stride, const int* seg_done_count, int seg_count,
              hipStream_t st) override {
        FusedArgs B = A;
        B.seg_done = (A.item_seg && A.unknown_seg) ? seg_done : nullptr;
        B.seg_stride = seg_stride;
        B.seg_done_count = seg_done_count;
        B.seg_gate = seg_count / 4 > 1 ? seg_count / 4 : 1;
        return fz_apply(B, reg, w, p, y, done, st);
    }
    void bytes(double* alg, double* phys, double* survey) override {
        // Algorithmic minimum of the matrix-free operator: every STORED entry of G and Q once (4 bytes:
        // the value; stored = the non-zero slots, counted by the set-up pass), the row -> cell map (4 bytes per row and level: the
        // only per-row index), one 27-entry stencil per cell (the column information, 108 bytes) and x, y once.
        // Physical: every dense slot once (zeros included), the row -> cell map, one 128-byte neighbour row per cell (sweep), the
        // slot-major per-cell sums written + read and the slot-major neighbour table (gather: 3 x 108 bytes per unknown), the
        // partial blocks of the cells that span workgroups written + read, x and y (+ x again for reg x).
        // SURVEY.md section 8d's formula prices an index per entry and both products: 2 x 8 bytes per stored entry + 12 M + 4.
        const double slots = 27.0 * A.depth * (double)A.rows_total;
        unsigned long long nnz = 0;                                  // (only reached with nksr_pcg_profile on, after a stream sync)
        if (A.nnz_counter) (void)hipMemcpy(&nnz, A.nnz_counter, sizeof(nnz), hipMemcpyDeviceToHost);
        const double stored = nnz > 0 ? (double)nnz : slots;
        *alg = 4.0 * stored + 4.0 * A.depth * (double)A.rows_total + (108.0 + 8.0) * A.M + 4.0;
        *phys = 4.0 * slots + 4.0 * A.depth * (double)A.rows_total + 2.0 * 128.0 * (double)A.nblocks + (128.0 + 3.0 * 108.0 + 12.0) * A.M;
        *survey = 2.0 * 8.0 * stored + 12.0 * A.M + 4.0;
        if (A.fac_vec) {
            // Factor form: the operator does not hold the entries of G and Q -- it rebuilds them.  Its minimum is what
            // defines it: one 16-byte record per row and level + one position record per row, the row -> cell map, and per cell the
            // 27-entry stencil (108 bytes), psi (16 bytes, every unknown's once), x and y.  Physical adds the 128-byte neighbour row
            // per cell, the slot-major per-cell sums written + read, the slot-major neighbour table and the partial blocks.
            const double rec = 16.0 * (A.depth + 1) * (double)A.rows_total + 4.0 * A.depth * (double)A.rows_total;
            *alg = rec + (108.0 + 16.0 + 8.0) * A.M + 4.0;
            *phys = rec + 2.0 * 128.0 * (double)A.nblocks + (128.0 + 16.0 + 3.0 * 108.0 + 12.0) * A.M;
        }
    }
};

extern "C" int nksr_pcg_solve_fused(const nksr_fused_op_t* opd, float reg, const float* diag, const float* b, float* x, float tol, int max_iter,
                                    int check_every, void* pcg_workspace, const nksr_coarse_precond_t* pc, const nksr_segments_t* seg,
                                    double* info_out, void* stream) {
    FusedOperator op;
    if (int rc = fz_args(op.A, opd)) return rc;
    if (op.A.M <= 0) { if (info_out) { info_out[0] = 0; info_out[1] = 0; } return NKSR_OK; }
    if (!pcg_workspace) return nksr_set_error(NKSR_ERR_ARG, "workspace is NULL");
    op.reg = reg;
    op.w = fz_carve(opd);
    return nksr_pcg_run(op, diag, op.A.M, b, x, tol, max_iter, check_every, pcg_workspace, info_out, (hipStream_t)stream, pc, seg);
}

extern "C" size_t nksr_pcg_vector_workspace_bytes(int32_t M) { return nksr_pcg_vector_bytes(M); }
