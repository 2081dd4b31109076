// What the conjugate-gradient driver (csrc/pcg.hip: CsrOperator) needs of the streaming CSR SpMV (csrc/spmv.hip).  Internal to the
// library: the symbols stay out of its dynamic table.
#pragma once
#include "common.h"

struct SpmvPlan {
    int nchunks;
    int32_t* chunk_row;   // [nchunks + 1]
    float* carry;         // [nchunks]
    int32_t* carry_row;   // [nchunks]
};

#pragma GCC visibility push(hidden)
// the plan's arrays inside a workspace of nksr_spmv_workspace_bytes(nnz) (filled by nksr_spmv_plan)
SpmvPlan carve_spmv(void* ws, int64_t nnz, int fmt);
// enqueue y = A x (the chunk kernel + the carry fix-up); `done` (device flag, may be NULL) != 0 turns both into no-ops
int launch_spmv(const int32_t* rowptr, const void* cols, const float* vals, int M, int64_t nnz, int fmt, const SpmvPlan& p,
                const float* x, float* y, const int* done, hipStream_t st);
// bytes one SpMV launch moves: algorithmic CSR figure of SURVEY.md section 8d (8 nnz + 12 M + 4) and what the physical
// layout actually streams (values + packed / int32 columns over the padded storage + row pointers + x + y)
void spmv_bytes(int M, int64_t nnz, int fmt, double* alg, double* phys);
#pragma GCC visibility pop
