// Device-wide primitives: radix sort, unique, exclusive sum.  These are plain library
// operations (rocPRIM through the hipCUB front-end); every domain kernel is hand-written.
#include "common.h"
#include <hipcub/hipcub.hpp>
#include <rocprim/rocprim.hpp>

// rocPRIM sorts up to 2^20 items by merge sort (block sort + log2(n / 1024) merge passes of two launches each: ~17 launches of 6-7 us
// for the 10^5-key streams of the coarser hierarchy levels and the mesh keys); with the bit range of a cloud's Morton keys (one
// onesweep pass per 8 varying bits) the onesweep path is fewer launches and less time from ~16 k items on.
using nksr_sort_config = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 16384>;
#include <stdarg.h>

thread_local char g_nksr_err[512] = "";

int nksr_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_nksr_err, sizeof(g_nksr_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char* nksr_last_error(void) { return g_nksr_err; }
extern "C" int nksr_version(void) { return 100; }

extern "C" int nksr_sort_keys_u64(void* tmp, size_t* tmp_bytes, const uint64_t* in, uint64_t* out, int64_t n,
                                  int begin_bit, int end_bit, void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    NKSR_CHECK_HIP(rocprim::radix_sort_keys<nksr_sort_config>(tmp, *tmp_bytes, in, out, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit, (hipStream_t)stream));
    return NKSR_OK;
}

extern "C" int nksr_sort_pairs_u64_u32(void* tmp, size_t* tmp_bytes, const uint64_t* kin, uint64_t* kout,
                                       const uint32_t* vin, uint32_t* vout, int64_t n, int begin_bit, int end_bit,
                                       void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    NKSR_CHECK_HIP(rocprim::radix_sort_pairs<nksr_sort_config>(tmp, *tmp_bytes, kin, kout, vin, vout, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit,
                                                               (hipStream_t)stream));
    return NKSR_OK;
}

extern "C" int nksr_unique_u64(void* tmp, size_t* tmp_bytes, const uint64_t* in, uint64_t* out, int64_t* d_count,
                               int64_t n, void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    NKSR_CHECK_HIP(hipcub::DeviceSelect::Unique(tmp, *tmp_bytes, in, out, d_count, n, (hipStream_t)stream));
    return NKSR_OK;
}

extern "C" int nksr_exclusive_sum_i32(void* tmp, size_t* tmp_bytes, const int32_t* in, int32_t* out, int64_t n,
                                      void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    NKSR_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, in, out, n, (hipStream_t)stream));
    return NKSR_OK;
}

extern "C" int nksr_exclusive_sum_i64(void* tmp, size_t* tmp_bytes, const int64_t* in, int64_t* out, int64_t n,
                                      void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    NKSR_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, in, out, n, (hipStream_t)stream));
    return NKSR_OK;
}

// ---- the run table of sorted keys (edges of a mesh, clusters of a simplification, voxels of a cloud) -----------------------------
// Position i HEADS a run when keys[i] < none_from and (i == 0 or keys[i - 1] != keys[i]); keys >= none_from (sorted: a tail) belong to
// no run.  Two passes of one lane per position around a scan of RUN_BLOCK-sized block counts: a ballot per wavefront, LDS only for the
// per-wave counts.
#define RUN_BLOCK 256

// heads of the block up to this lane's wavefront in s[], returns whether this lane's position is a head; every lane must call it
__device__ __forceinline__ bool run_head(const uint64_t* __restrict__ keys, int64_t i, int64_t n, uint64_t none_from, unsigned long long& wave_heads,
                                         int* s) {
    bool head = false;
    if (i < n) {
        const uint64_t k = keys[i];
        head = k < none_from && (i == 0 || keys[i - 1] != k);
    }
    wave_heads = __ballot(head);
    if ((threadIdx.x & (NKSR_WAVE - 1)) == 0) s[threadIdx.x / NKSR_WAVE] = __popcll(wave_heads);
    __syncthreads();
    return head;
}

__global__ void __launch_bounds__(RUN_BLOCK) k_run_counts(const uint64_t* __restrict__ keys, int64_t n, uint64_t none_from,
                                                          int64_t* __restrict__ counts, int64_t nb) {
    __shared__ int s[RUN_BLOCK / NKSR_WAVE];
    unsigned long long m;
    run_head(keys, (int64_t)blockIdx.x * RUN_BLOCK + threadIdx.x, n, none_from, m, s);
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < RUN_BLOCK / NKSR_WAVE; ++w) t += s[w];
        counts[blockIdx.x] = t;
        if (blockIdx.x == 0) counts[nb] = 0;
    }
}

// run r = rank of its head: start[r] = the head's position, run_key[r] its key; start[n_runs] = the position of the first key >=
// none_from, or n; run_of[i] = the heads up to and including i, minus one (-1 behind none_from)
__global__ void __launch_bounds__(RUN_BLOCK) k_run_table(const uint64_t* __restrict__ keys, int64_t n, uint64_t none_from,
                                                         const int64_t* __restrict__ offsets, int64_t n_runs, uint32_t* __restrict__ start,
                                                         uint64_t* __restrict__ run_key, int32_t* __restrict__ run_of) {
    __shared__ int s[RUN_BLOCK / NKSR_WAVE];
    const int64_t i = (int64_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    unsigned long long m;
    const bool head = run_head(keys, i, n, none_from, m, s);
    if (i >= n) return;
    const int lane = threadIdx.x & (NKSR_WAVE - 1), wave = threadIdx.x / NKSR_WAVE;
    int upto = __popcll(m & ((2ull << lane) - 1ull));               // heads of this wavefront up to and including this lane
    for (int w = 0; w < wave; ++w) upto += s[w];
    const int64_t r = offsets[blockIdx.x] + upto - 1;
    const uint64_t k = keys[i];
    const bool in_run = k < none_from && r >= 0 && r < n_runs;      // (r outside [0, n_runs): offsets that are not the scan of these keys)
    if (head && in_run) {
        start[r] = (uint32_t)i;
        if (run_key) run_key[r] = k;
    }
    if (run_of) run_of[i] = in_run ? (int32_t)r : -1;
    if (k >= none_from ? (i == 0 || keys[i - 1] < none_from) : i == n - 1) start[n_runs] = (uint32_t)(k >= none_from ? i : n);
}

static int run_check(const char* who, int64_t n) {
    if (n < 0) return nksr_set_error(NKSR_ERR_ARG, "%s: negative size (n=%lld)", who, (long long)n);
    if (n >= (1ll << 32)) return nksr_set_error(NKSR_ERR_ARG, "%s: n=%lld, at most 2^32 - 1 keys (run starts are uint32)", who, (long long)n);
    return NKSR_OK;
}

extern "C" int64_t nksr_run_blocks(int64_t n) { return n > 0 ? (n + RUN_BLOCK - 1) / RUN_BLOCK : 0; }

extern "C" int nksr_run_counts_u64(const uint64_t* keys_sorted, int64_t n, uint64_t none_from, int64_t* block_counts, void* stream) {
    int rc = run_check("run counts", n);
    if (rc) return rc;
    if (!block_counts || (n > 0 && !keys_sorted)) return nksr_set_error(NKSR_ERR_ARG, "run counts: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { NKSR_CHECK_HIP(hipMemsetAsync(block_counts, 0, sizeof(int64_t), st)); return NKSR_OK; }
    const int64_t nb = nksr_run_blocks(n);
    hipLaunchKernelGGL(k_run_counts, dim3((unsigned)nb), dim3(RUN_BLOCK), 0, st, keys_sorted, n, none_from, block_counts, nb);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_run_table_u64(const uint64_t* keys_sorted, int64_t n, uint64_t none_from, const int64_t* block_offsets, int64_t n_runs,
                                  uint32_t* start_out, uint64_t* run_key_out, int32_t* run_of_out, void* stream) {
    int rc = run_check("run table", n);
    if (rc) return rc;
    if (n_runs < 0 || n_runs > n) return nksr_set_error(NKSR_ERR_ARG, "run table: n_runs=%lld of %lld keys", (long long)n_runs, (long long)n);
    if (run_of_out && n_runs >= (1ll << 31))
        return nksr_set_error(NKSR_ERR_ARG, "run table: n_runs=%lld, at most 2^31 - 1 runs with run_of_out (int32)", (long long)n_runs);
    if (!start_out || (n > 0 && (!keys_sorted || !block_offsets))) return nksr_set_error(NKSR_ERR_ARG, "run table: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { NKSR_CHECK_HIP(hipMemsetAsync(start_out, 0, sizeof(uint32_t), st)); return NKSR_OK; }
    hipLaunchKernelGGL(k_run_table, dim3((unsigned)nksr_run_blocks(n)), dim3(RUN_BLOCK), 0, st, keys_sorted, n, none_from, block_offsets, n_runs,
                       start_out, run_key_out, run_of_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// the sampler's area CDF: rocPRIM's deterministic look-back, so the fp64 sums (and with them every sample) repeat bit for bit
extern "C" int nksr_inclusive_sum_f64(void* tmp, size_t* tmp_bytes, const double* in, double* out, int64_t n, void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    if (n < 0) return nksr_set_error(NKSR_ERR_ARG, "inclusive sum: negative size");
    if (tmp && n > 0 && (!in || !out)) return nksr_set_error(NKSR_ERR_ARG, "inclusive sum: NULL arrays");
    NKSR_CHECK_HIP(rocprim::deterministic_inclusive_scan(tmp, *tmp_bytes, in, out, (size_t)n, rocprim::plus<double>(), (hipStream_t)stream));
    return NKSR_OK;
}

// per-component area sums (mesh topology): the same deterministic look-back, restarted wherever the (sorted) key changes, so a
// segment's last element holds the sum of that segment alone -- no difference of two long prefix sums
extern "C" int nksr_inclusive_sum_by_key_f64(void* tmp, size_t* tmp_bytes, const uint64_t* keys, const double* in, double* out, int64_t n,
                                             void* stream) {
    if (!tmp_bytes) return nksr_set_error(NKSR_ERR_ARG, "tmp_bytes is NULL");
    if (n < 0) return nksr_set_error(NKSR_ERR_ARG, "inclusive sum by key: negative size");
    if (tmp && n > 0 && (!keys || !in || !out)) return nksr_set_error(NKSR_ERR_ARG, "inclusive sum by key: NULL arrays");
    NKSR_CHECK_HIP(rocprim::deterministic_inclusive_scan_by_key(tmp, *tmp_bytes, keys, in, out, (size_t)n, rocprim::plus<double>(),
                                                                rocprim::equal_to<uint64_t>(), (hipStream_t)stream));
    return NKSR_OK;
}
