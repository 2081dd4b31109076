// Steps 4' of the packed coarse block (csrc/assemble.hip: nksr_assemble_packed leaves every row's kept own words, kept mirror words and
// counts): the kept mirror words compacted to a dense list (ascending source row), sorted by the caller stably on the destination
// bits alone (keys only, a seventh of the entries at 8 instead of 12 bytes), and k_pk_rows writes every row  [mirrors][lower][upper]
// in the new order: word for word what nksr_coarse_pack makes of the fp32 CSR, which is never written.
#include "common.h"

// kept mirror words of row r: [mir_off[r], + kept[r]) of the structural list -> [kept_off[r], ...) of the dense one.  16 lanes per row.
__global__ void __launch_bounds__(256) k_pk_compact(int M, const uint64_t* __restrict__ staged, const int32_t* __restrict__ mir_off,
                                                    const int32_t* __restrict__ kept, const int32_t* __restrict__ kept_off,
                                                    uint64_t* __restrict__ dense) {
    const int r = (blockIdx.x * 256 + threadIdx.x) >> 4, l = threadIdx.x & 15;
    if (r >= M) return;
    const int n = kept[r], src = mir_off[r], dst = kept_off[r];
    for (int k = l; k < n; k += 16) dense[dst + k] = staged[src + k];
}

// run [runs[d], runs[n + d]) of destination row d in the sorted mirror words (both zero where a row has none: cleared by the caller)
__global__ void __launch_bounds__(256) k_pk_runs(const uint64_t* __restrict__ sorted, int nk, int n, int32_t* __restrict__ runs) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= nk) return;
    const int d = (int)(sorted[m] >> 32);
    if (m == 0 || (int)(sorted[m - 1] >> 32) != d) runs[d] = m;
    if (m == nk - 1 || (int)(sorted[m + 1] >> 32) != d) runs[n + d] = m + 1;
}

__global__ void __launch_bounds__(256) k_pk_lens(int n, const int32_t* __restrict__ runs, const int32_t* __restrict__ kept,
                                                 const int32_t* __restrict__ old_of_new, int32_t* __restrict__ lens) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int o = old_of_new[i];
    lens[i] = (runs[n + i] - runs[i]) + kept[o] + kept[(int64_t)(n + 1) + o];
}

// row i of the packed block (new order) = [kept mirrors, ascending source row][kept same-level lower][kept own upper] -- the order
// k_cc_pack (csrc/cheb.hip) leaves of the CSR row -- and dis[i] = D^-1/2.  16 lanes per row.
__global__ void __launch_bounds__(256) k_pk_rows(int n, const uint64_t* __restrict__ sorted, const int32_t* __restrict__ runs,
                                                 const uint32_t* __restrict__ own, const int32_t* __restrict__ own_off,
                                                 const int32_t* __restrict__ samelow, const int32_t* __restrict__ kept,
                                                 const int32_t* __restrict__ old_of_new, const int32_t* __restrict__ prow,
                                                 const float* __restrict__ diag, uint32_t* __restrict__ pk, float* __restrict__ dis) {
    const int i = (blockIdx.x * 256 + threadIdx.x) >> 4, l = threadIdx.x & 15;
    if (i >= n) return;
    const int o = old_of_new[i];
    int p = prow[i];
    const int mb = runs[i], nm = runs[n + i] - mb;
    for (int k = l; k < nm; k += 16) pk[p + k] = (uint32_t)sorted[mb + k];
    p += nm;
    const int lo = own_off[o], nl = kept[o], nu = kept[(int64_t)(n + 1) + o];
    for (int k = l; k < nl; k += 16) pk[p + k] = own[lo + k];
    p += nl;
    const int up = lo + samelow[o];
    for (int k = l; k < nu; k += 16) pk[p + k] = own[up + k];
    if (l == 0) dis[i] = 1.f / sqrtf(diag[o]);
}

extern "C" int nksr_packed_mirrors_compact(int32_t n, const uint64_t* mir_staged, const int32_t* mir_off, const int32_t* kept_mir,
                                           const int32_t* kept_off, uint64_t* mir_dense, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!mir_staged || !mir_off || !kept_mir || !kept_off || !mir_dense) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    hipLaunchKernelGGL(k_pk_compact, dim3(nksr_blocks((int64_t)n * 16, 256)), dim3(256), 0, (hipStream_t)stream, n, mir_staged, mir_off,
                       kept_mir, kept_off, mir_dense);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_packed_row_lengths(int32_t n, const uint64_t* mir_sorted, int64_t n_mir, const int32_t* kept, const int32_t* old_of_new,
                                       int32_t* runs_out, int32_t* lens_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if ((n_mir > 0 && !mir_sorted) || !kept || !old_of_new || !runs_out || !lens_out) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    if (n_mir < 0 || n_mir >= ((int64_t)1 << 31)) return nksr_set_error(NKSR_ERR_ARG, "bad mirror count");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(runs_out, 0, 2 * (size_t)n * sizeof(int32_t), st));
    if (n_mir > 0) hipLaunchKernelGGL(k_pk_runs, dim3(nksr_blocks(n_mir, 256)), dim3(256), 0, st, mir_sorted, (int)n_mir, n, runs_out);
    hipLaunchKernelGGL(k_pk_lens, dim3(nksr_blocks(n, 256)), dim3(256), 0, st, n, (const int32_t*)runs_out, kept, old_of_new, lens_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_packed_rows(int32_t n, const uint64_t* mir_sorted, const int32_t* runs, const uint32_t* own, const int32_t* own_off,
                                const int32_t* samelow, const int32_t* kept, const int32_t* old_of_new, const int32_t* packed_rowptr,
                                const float* diag, uint32_t* packed_out, float* dis_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!runs || !own || !own_off || !samelow || !kept || !old_of_new || !packed_rowptr || !diag || !packed_out || !dis_out)
        return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    hipLaunchKernelGGL(k_pk_rows, dim3(nksr_blocks((int64_t)n * 16, 256)), dim3(256), 0, (hipStream_t)stream, n, mir_sorted, runs, own, own_off,
                       samelow, kept, old_of_new, packed_rowptr, diag, packed_out, dis_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
