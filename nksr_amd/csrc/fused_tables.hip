// Tables of the matrix-free operator, built once per solve.  All they need is row_cells[d][r], written
// by nksr_kernel_rows next to the rows: the sites are Morton-sorted, so the rows of a cell are one contiguous run at every level.
//   span       first / last row of every cell (-1: the cell has no rows) and the first workgroup of the sweep that reaches it
//   item_begin the row list cut into the sweep's work items, aligned to unit boundaries (k_fz_item_begin)
//   counts     partial blocks of every cell: one per workgroup its rows reach into, none for a cell inside one workgroup; the caller
//              scans them into offsets (fields/operator_setup.py)
//   nbr32      per unknown, row-major: its 27 neighbours, block base and row span -- what the sweep (csrc/fused_sweep.hip) reads per cell
//   nbrT       the 27 neighbours slot-major -- what the gather (csrc/fused.hip) reads with one lane per unknown
#include "fused_dev.h"
#include "hier_dev.h"

// span[0][j] / span[1][j]: first / last row of cell j (-1 = the cell has no rows)
__global__ void k_fz_spans(int depth, int64_t rows_total, const int32_t* __restrict__ row_cells, int32_t* __restrict__ first,
                           int32_t* __restrict__ last) {
    const int64_t lin = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lin >= rows_total * depth) return;
    const int64_t r = lin % rows_total;
    const int c = row_cells[lin];
    if (c < 0) return;
    if (r == 0 || row_cells[lin - 1] != c) first[c] = (int32_t)r;
    if (r == rows_total - 1 || row_cells[lin + 1] != c) last[c] = (int32_t)r;
}

// A UNIT = a maximal run of rows that lie in the same cell at every level (the rows of one level-0 cell, as a rule).  Item i of the
// sweep = the units that start in the 32-row window [32 i, 32 i + 32): rows [item_begin[i], item_begin[i + 1]) -- variable length,
// aligned to unit boundaries; an item is empty when a long unit covers its window.  Eight items are a workgroup.
__global__ void k_fz_item_begin(int depth, int64_t rows_total, int nitems, int nentries, const int32_t* __restrict__ row_cells,
                                int32_t* __restrict__ item_begin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nentries) return;
    int64_t r = (int64_t)i * FZ_RC;
    if (i >= nitems || r >= rows_total) { item_begin[i] = (int32_t)rows_total; return; }
    while (r > 0 && r < rows_total) {
        bool start = false;
        for (int d = 0; d < depth; ++d) start = start || row_cells[(int64_t)d * rows_total + r] != row_cells[(int64_t)d * rows_total + r - 1];
        if (start) break;
        ++r;
    }
    item_begin[i] = (int32_t)r;
}
// workgroup of the sweep that processes row r: the last w with item_begin[8 w] <= r
__device__ __forceinline__ int fz_wg_of(const int32_t* __restrict__ item_begin, int nwg, int r) {
    int lo = 0, hi = nwg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (item_begin[mid * FZ_HW] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// partial blocks of a cell: one per workgroup its rows reach into -- if that is more than one; a cell inside one workgroup has none
// (the sweep finishes it)
__global__ void k_fz_block_counts(int M, int nwg, const int32_t* __restrict__ item_begin, const int32_t* __restrict__ first,
                                  const int32_t* __restrict__ last, int32_t* __restrict__ wgfirst, int32_t* __restrict__ counts) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > M) return;
    int n = 0;
    if (j < M) {
        int w0 = 0;
        if (first[j] >= 0) {
            w0 = fz_wg_of(item_begin, nwg, first[j]);
            n = fz_wg_of(item_begin, nwg, last[j]) - w0 + 1;
            if (n == 1) n = 0;
        }
        wgfirst[j] = w0;
    }
    counts[j] = n;
}

// nbr32[j][0..26]: global unknown index of the neighbour voxels or -1;  [27]: (first block of j) - (first workgroup of j), so that
// the block of workgroup w is nbr32[j][27] + w;  [28] / [29]: first / last row of the cell (-1: none);  [30] / [31]: unused (0)
// One workgroup per 64 unknowns writes BOTH tables from one read of the hierarchy's neighbour rows: nbr32 row-major as it is formed,
// nbrT slot-major out of an LDS tile (two kernels that read the rows, then nbr32 again, took 3.7 + 1.4 ms per scene step).
__global__ void __launch_bounds__(256) k_fz_tables(nksr_hier_t hier, int M, const int32_t* __restrict__ offsets, const int32_t* __restrict__ first,
                                                   const int32_t* __restrict__ last, const int32_t* __restrict__ wgfirst,
                                                   int32_t* __restrict__ nbr32, int32_t* __restrict__ nbrT) {
    __shared__ int32_t tile[64][33];
    const int j0 = blockIdx.x * 64;
    for (int i = threadIdx.x; i < 64 * 32; i += 256) {
        const int jj = i >> 5, s = i & 31, j = j0 + jj;
        int v = -1;
        if (j < M) {
            v = 0;
            if (s < 27) {
                const int d = row_level(hier, j), c = j - hier.lv[d].offset;
                const int nb = hier.lv[d].nbr[(int64_t)c * 27 + s];
                v = nb >= 0 ? nb + hier.lv[d].offset : -1;
            } else if (s == 27) {
                v = offsets[j] - wgfirst[j];
            } else if (s == 28) {
                v = first[j];
            } else if (s == 29) {
                v = last[j];
            }
        }
        tile[jj][s] = v;
        if (j < M) nbr32[(int64_t)j * 32 + s] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 27 * 64; i += 256) {
        const int s = i >> 6, jj = i & 63;
        if (j0 + jj < M) nbrT[(int64_t)s * M + j0 + jj] = tile[jj][s];
    }
}

extern "C" int64_t nksr_fused_item_entries(int64_t rows_total) { return (int64_t)fz_nwg(rows_total) * FZ_HW + 1; }
extern "C" int64_t nksr_fused_count_words(int64_t rows_total) { return (int64_t)fz_nwg(rows_total) + 1; }

extern "C" int nksr_fused_block_counts(int32_t depth, int32_t M, int64_t rows_total, const int32_t* row_cells, int32_t* span_out,
                                       int32_t* item_begin_out, int32_t* counts_out, void* stream) {
    if (depth < 1 || depth > NKSR_MAX_DEPTH) return nksr_set_error(NKSR_ERR_ARG, "bad depth %d", depth);
    if (M <= 0) return NKSR_OK;
    if (rows_total < 0 || rows_total >= ((int64_t)1 << 31) - 2 * FZ_WG_ROWS) return nksr_set_error(NKSR_ERR_CAPACITY, "too many kernel rows");
    if (!span_out || !counts_out || !item_begin_out || (rows_total > 0 && !row_cells)) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(span_out, 0xFF, (size_t)2 * M * sizeof(int32_t), st));
    const int nent = (int)nksr_fused_item_entries(rows_total);
    hipLaunchKernelGGL(k_fz_item_begin, dim3(nksr_blocks(nent, 256)), dim3(256), 0, st, depth, rows_total, fz_items(rows_total), nent, row_cells, item_begin_out);
    if (rows_total > 0)
        hipLaunchKernelGGL(k_fz_spans, dim3(nksr_blocks(rows_total * depth, 256)), dim3(256), 0, st, depth, rows_total, row_cells, span_out, span_out + M);
    hipLaunchKernelGGL(k_fz_block_counts, dim3(nksr_blocks((int64_t)M + 1, 256)), dim3(256), 0, st, M, fz_nwg(rows_total) > 0 ? fz_nwg(rows_total) : 1,
                       (const int32_t*)item_begin_out, (const int32_t*)span_out, (const int32_t*)(span_out + M), span_out + 2 * (int64_t)M, counts_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_fused_tables(const nksr_hier_t* h, int64_t rows_total, const int32_t* item_begin, const int32_t* offsets, const int32_t* span,
                                 int32_t* nbr32_out, int32_t* nbrT_out, void* stream) {
    if (!h || h->depth < 1 || h->depth > NKSR_MAX_DEPTH) return nksr_set_error(NKSR_ERR_ARG, "bad hierarchy");
    const int M = h->lv[h->depth - 1].offset + h->lv[h->depth - 1].n;
    if (M <= 0) return NKSR_OK;
    if (!offsets || !span || !nbr32_out || !nbrT_out || !item_begin) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    hipLaunchKernelGGL(k_fz_tables, dim3(nksr_blocks(M, 64)), dim3(256), 0, (hipStream_t)stream, *h, M, offsets, span, span + M,
                       span + 2 * (int64_t)M, nbr32_out, nbrT_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
