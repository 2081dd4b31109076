// What the three parts of the assembly share: the arguments every kernel takes, the carve of the workspace
// they point into, the physical CSR slot and the scratch one level's split Gram blocks need.  csrc/gram.hip forms the per-cell Gram
// blocks (phase 1), csrc/assemble.hip counts the structure and fills the rows from them (phase 2).  Internal to the library: the
// symbols stay out of its dynamic table.  (Not in common.h: build.kernel_hash covers that file for the roofline kernels.)
#pragma once
#include "common.h"
#include "hier_dev.h"
#include <type_traits>

#define ASM_WAVES 1

struct AsmArgs {
    nksr_hier_t hier;
    nksr_siteset_t sets[3];
    int nsets;
    int M;
    int col_bits;
    float reg;
    float* blocks[NKSR_MAX_DEPTH];   // [n_d, 27, T_d]
    float* bvec[NKSR_MAX_DEPTH];     // [n_d, 27]
    int32_t* nsites[NKSR_MAX_DEPTH]; // [n_d]
    int32_t* colmap[NKSR_MAX_DEPTH]; // [n_d, (L-d) 125] column of every structural upper slot or -1
    int col_format;                  // physical layout of cols_out / vals_out (csr_phys)
};

// bytes of level d's blocks, bvec, nsites and colmap inside the workspace, each rounded up to 256: the arrays follow each other in
// this order, level after level (fill_args places them, nksr_assemble_workspace_bytes adds them up)
struct AsmCarve { size_t blocks, bvec, nsites, colmap; };
static inline AsmCarve asm_carve(const nksr_hier_t* h, int d) {
    const size_t n = (size_t)h->lv[d].n, levels = (size_t)(h->depth - d);
    auto up = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    return {up(n * 27 * levels * 27 * sizeof(float)), up(n * 27 * sizeof(float)), up(n * sizeof(int32_t)), up(n * levels * 125 * sizeof(int32_t))};
}

// Bytes of split scratch the parallel schedule of a level needs (csrc/gram.hip): the raw accumulator, NT tiles of 16 x 64 floats, of
// every (cell, part).  0: the level does not split, or has more than ~64 k (cell, part) wavefronts -- it runs the sequential schedule.
static inline size_t asm_split_bytes(int n, int parts, size_t NT) {
    if (n <= 0 || parts <= 1 || (int64_t)n * parts > 65536) return 0;
    return (size_t)n * parts * NT * 16 * 64 * sizeof(float);
}

// f(std::integral_constant<int, N>) with N = v clamped to [1, MAX]: a run-time tile or vector width as a template argument
template <int MAX, class F>
static inline void asm_with_width(int v, F&& f) {
    if constexpr (MAX > 1) {
        if (v < MAX) return asm_with_width<MAX - 1>(v, f);
    }
    f(std::integral_constant<int, MAX>{});
}

// physical CSR layout (see csrc/spmv.hip): tiles of 64 EPL entries, logical entry m of a tile at
// EPL (m % 64) + m / 64;  EPL = 4 (col_format 0, 256-entry tiles) or 3 (col_format 1, 192-entry tiles); col_format 2 = plain CSR
// order (the small coarse-level block of the PCG's preconditioner, csrc/cheb.hip)
__device__ __forceinline__ int64_t csr_phys(int64_t k, int fmt) {
    if (fmt == 2) return k;
    if (fmt == 0) {
        const int64_t m = k & 255;
        return (k & ~(int64_t)255) + 4 * (m & 63) + (m >> 6);
    }
    const uint32_t kk = (uint32_t)k;               // nnz < 2^31: 32-bit magic-number division, not the 64-bit expansion
    const uint32_t t = kk / 192u, m = kk - t * 192u;
    return (int64_t)(t * 192u + 3u * (m & 63u) + (m >> 6));
}

#pragma GCC visibility push(hidden)
// phase 1 of every level (csrc/gram.hip): checks the site sets against the hierarchy, then blocks / bvec / nsites of every cell
int launch_cell_blocks(const AsmArgs& A, const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, void* split_scratch,
                       size_t split_scratch_bytes, hipStream_t st);
#pragma GCC visibility pop
