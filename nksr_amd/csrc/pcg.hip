// Jacobi-preconditioned conjugate gradients on the CSR normal equations.  The solve is three translation units:
//   spmv.hip  the streaming CSR SpMV y = A p -- the roofline kernel; build.kernel_hash('spmv') covers that file,
//             spmv.h and common.h and nothing of the two below
//   cheb.hip  the coarse-level block preconditioner in both of its formats: Chebyshev steps, eigenvalue bounds, the CSR -> packed
//             converter (drop rule and entry word: coarse_pack_dev.h, shared with assemble.hip)
//   pcg.hip   this file: the segmented conjugate-gradient loop (nksr_pcg_run, which fused.hip -- the matrix-free operator: fused_tables.hip, fused_sweep.hip, fused.hip -- drives with its own operator through
//             pcg_core.h), its workspace, the live profiling of the operator launches, and the CSR solve nksr_pcg_solve
// pcg_dev.h holds what the loop and the preconditioner share: SegScalars and the fixed-order reductions.
// Per iteration: (1) y = A p, (2) partial dot p.y (own small kernel, see k_spcg_dot), (3) x,r,z update
// fused with the partial dots r.r and r.z, (4) p update.  alpha/beta never leave the device; dot products are
// accumulated in fp64 with a fixed reduction order (deterministic).  A device-side `done` flag
// turns the remaining launches of a chunk into no-ops, so the host only syncs every
// `check_every` iterations.
#include "common.h"
#include "pcg_core.h"
#include "pcg_dev.h"
#include "spmv.h"
#include "cheb.h"
#include <mutex>
#include <vector>

#define SPCG_BS 1024            // unknowns per reduction block of the segmented PCG (256 threads x 4)

struct PcgGlobal {          // what the host reads back every check_every iterations
    double max_rel;
    int max_iter;
    int done_all;
    int done_count;
    int nblocks;            // reduction blocks in use (k_seg_fill)
    int min_iter;           // fewest iterations any segment has taken so far (= all segments were still iterating up to here)
    int fallbacks;          // segments that dropped the coarse-level block and went on with Jacobi
    int pad;
};

struct PcgWork {
    float *r, *z, *p, *y;
    double* part1;          // [nb_max]
    double* part2;          // [3 * nb_max]: r.r, r.z with the preconditioner in use, r.z with plain Jacobi (the fallback's)
    int32_t *blk_lo, *blk_hi, *blk_seg;   // [nb_max] reduction blocks: unknown range + segment
    int32_t* seg_blk;       // [nseg + 1] first block of every segment
    SegScalars* sc;         // [nseg]
    PcgGlobal* g;
    int nseg, nranges, nb_max;
    const int32_t *lo, *hi; // [nseg * nranges] (device) or NULL: one segment [0, M)
    int M;
};

static int spcg_nb_max(int32_t M, int nseg, int nranges) { return (M + SPCG_BS - 1) / SPCG_BS + nseg * nranges; }

static size_t pcg_vector_bytes_seg(int32_t M, int nseg, int nranges) {
    const size_t vec = align_up((size_t)M * sizeof(float), 256), nb = (size_t)spcg_nb_max(M, nseg, nranges);
    return 4 * vec + align_up(4 * nb * sizeof(double), 256) + align_up(3 * nb * sizeof(int32_t), 256) + align_up(((size_t)nseg + 1) * sizeof(int32_t), 256) +
           align_up((size_t)nseg * sizeof(SegScalars), 256) + 256;
}
static size_t pcg_vector_bytes(int32_t M) { return pcg_vector_bytes_seg(M, 1, 1); }
size_t nksr_pcg_vector_bytes(int32_t M) { return pcg_vector_bytes(M); }
extern "C" size_t nksr_pcg_vector_workspace_bytes_seg(int32_t M, int32_t nseg, int32_t nranges) {
    return pcg_vector_bytes_seg(M, nseg < 1 ? 1 : nseg, nranges < 1 ? 1 : nranges);
}
extern "C" size_t nksr_pcg_workspace_bytes(int32_t M, int64_t nnz) {
    return pcg_vector_bytes(M) + nksr_spmv_workspace_bytes(nnz);
}

static PcgWork carve(void* ws, int M, const nksr_segments_t* seg) {
    PcgWork w;
    w.nseg = seg ? seg->nseg : 1;
    w.nranges = seg ? seg->nranges : 1;
    w.lo = seg ? seg->lo : nullptr;
    w.hi = seg ? seg->hi : nullptr;
    w.M = M;
    w.nb_max = spcg_nb_max(M, w.nseg, w.nranges);
    char* p = (char*)ws;
    const size_t vec = align_up((size_t)M * sizeof(float), 256), nb = (size_t)w.nb_max;
    w.r = (float*)p; p += vec;
    w.z = (float*)p; p += vec;
    w.p = (float*)p; p += vec;
    w.y = (float*)p; p += vec;
    w.part1 = (double*)p;
    w.part2 = w.part1 + nb; p += align_up(4 * nb * sizeof(double), 256);
    w.blk_lo = (int32_t*)p;
    w.blk_hi = w.blk_lo + nb;
    w.blk_seg = w.blk_hi + nb; p += align_up(3 * nb * sizeof(int32_t), 256);
    w.seg_blk = (int32_t*)p; p += align_up(((size_t)w.nseg + 1) * sizeof(int32_t), 256);
    w.sc = (SegScalars*)p; p += align_up((size_t)w.nseg * sizeof(SegScalars), 256);
    w.g = (PcgGlobal*)p;
    return w;
}

// ---- reduction-block plan of the segmented PCG ------------------------------------------------------------------------------
__device__ __forceinline__ void seg_range(const PcgWork& w, int c, int k, int& lo, int& hi) {
    if (w.lo) { lo = w.lo[c * w.nranges + k]; hi = w.hi[c * w.nranges + k]; } else { lo = 0; hi = w.M; }
    if (hi < lo) hi = lo;
}
__device__ __forceinline__ int seg_range_blocks(const PcgWork& w, int c, int k) {
    int lo, hi;
    seg_range(w, c, k, lo, hi);
    return (hi - lo + SPCG_BS - 1) / SPCG_BS;
}
__global__ void k_seg_count(PcgWork w) {          // one thread per segment
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.nseg) return;
    int n = 0;
    for (int k = 0; k < w.nranges; ++k) n += seg_range_blocks(w, c, k);
    w.seg_blk[c + 1] = n;
}
__global__ void k_seg_scan(PcgWork w) {           // a few thousand segments at most: one thread
    int acc = 0;
    w.seg_blk[0] = 0;
    for (int c = 0; c < w.nseg; ++c) { acc += w.seg_blk[c + 1]; w.seg_blk[c + 1] = acc; }
    w.g->nblocks = acc;
    w.g->done_all = 0;
    w.g->done_count = 0;
    w.g->max_iter = 0;
    w.g->max_rel = 1.0;
}
__global__ void k_seg_fill(PcgWork w) {           // one wavefront per (segment, range)
    const int idx = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (idx >= w.nseg * w.nranges) return;
    const int c = idx / w.nranges, k = idx - c * w.nranges;
    int base = w.seg_blk[c];
    for (int q = 0; q < k; ++q) base += seg_range_blocks(w, c, q);
    int lo, hi;
    seg_range(w, c, k, lo, hi);
    const int nb = (hi - lo + SPCG_BS - 1) / SPCG_BS;
    for (int j = lane; j < nb; j += 64) {
        const int s = lo + j * SPCG_BS;
        w.blk_lo[base + j] = s;
        w.blk_hi[base + j] = s + SPCG_BS < hi ? s + SPCG_BS : hi;
        w.blk_seg[base + j] = c;
    }
}

// a segment finished (converged / empty / broke down): the launch-wide flag goes up when all have
__device__ __forceinline__ void seg_retire(PcgWork& w) {
    if (atomicAdd(&w.g->done_count, 1) + 1 == w.nseg) w.g->done_all = 1;
}

#define SPCG_BLOCK_PROLOGUE(check_done)                                \
    const int blk = blockIdx.x;                                        \
    if (blk >= w.g->nblocks) return;                                   \
    const int seg = w.blk_seg[blk];                                    \
    if ((check_done) && w.sc[seg].done) return;                        \
    const int lo = w.blk_lo[blk], hi = w.blk_hi[blk];                  \
    __shared__ double sm[PCG_BLOCK / 64];

__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_init(PcgWork w, const float* __restrict__ b, const float* __restrict__ diag,
                                                         float* __restrict__ x) {
    SPCG_BLOCK_PROLOGUE(false)
    double bb = 0.0, rz = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += PCG_BLOCK) {
        const float bi = b[i];
        const float zi = bi / diag[i];
        x[i] = 0.f;
        w.r[i] = bi;
        w.z[i] = zi;
        w.p[i] = zi;
        bb += (double)bi * bi;
        rz += (double)bi * zi;
    }
    const double t0 = block_sum(bb, sm);
    const double t1 = block_sum(rz, sm);
    if (threadIdx.x == 0) {
        w.part2[3 * blk] = t0;
        w.part2[3 * blk + 1] = t1;
        w.part2[3 * blk + 2] = t1;
    }
}

// one workgroup per segment.  r.z <= 0 with the coarse-level block in z (the Chebyshev polynomial lost definiteness: eigenvalue
// bound too small) while the Jacobi r.z is positive: the segment starts with Jacobi alone (p = z = r / diag) instead of failing.
__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_init_finish(PcgWork w, const float* __restrict__ diag) {
    __shared__ double sm[PCG_BLOCK / 64];
    const int c = blockIdx.x, b0 = w.seg_blk[c], nb = w.seg_blk[c + 1] - b0;
    const double bb = reduce_partials(w.part2 + 3 * (int64_t)b0, nb, 3, sm);
    const double rz = reduce_partials(w.part2 + 3 * (int64_t)b0 + 1, nb, 3, sm);
    const double rzj = reduce_partials(w.part2 + 3 * (int64_t)b0 + 2, nb, 3, sm);
    const bool fall = bb != 0.0 && !(rz > 0.0) && rzj > 0.0;
    if (fall)
        for (int k = 0; k < nb; ++k)
            for (int i = w.blk_lo[b0 + k] + threadIdx.x; i < w.blk_hi[b0 + k]; i += PCG_BLOCK) { const float zi = w.r[i] / diag[i]; w.z[i] = zi; w.p[i] = zi; }
    if (threadIdx.x == 0) {
        SegScalars& s = w.sc[c];
        s.bb = bb;
        s.rz[0] = fall ? rzj : rz;
        s.rz[1] = 0.0;
        s.rel = bb == 0.0 ? 0.0 : 1.0;
        s.iter = 0;
        s.done = 0;
        s.jacobi = fall ? 1 : 0;
        s.pad = 0;
        if (bb == 0.0 || !(s.rz[0] > 0.0)) { s.done = bb == 0.0 ? 1 : 2; seg_retire(w); }      // empty / zero right-hand side; 2 = breakdown
    }
}

// partial sums of p.Ap (fp64, fixed order).  Kept out of the operator on purpose: fused into the SpMV, lane 0 of every
// wavefront waited for a dependent x[r] load once per row, which cost the SpMV ~10 % (761 vs 680 us).
__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_dot(PcgWork w) {
    SPCG_BLOCK_PROLOGUE(true)
    double acc = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += PCG_BLOCK) acc += (double)w.p[i] * (double)w.y[i];
    const double t = block_sum(acc, sm);
    if (threadIdx.x == 0) w.part1[blk] = t;
}

// x += alpha p ; r -= alpha y ; z = r / diag ; partial r.r and r.z   (alpha of the block's segment)
__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_update(PcgWork w, const float* __restrict__ diag, float* __restrict__ x, int parity) {
    SPCG_BLOCK_PROLOGUE(true)
    const int b0 = w.seg_blk[seg];
    const double pAp = reduce_partials(w.part1 + b0, w.seg_blk[seg + 1] - b0, 1, sm);
    const float alpha = pAp > 0.0 ? (float)(w.sc[seg].rz[parity] / pAp) : 0.f;
    double rr = 0.0, rz = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += PCG_BLOCK) {
        const float pi = w.p[i], yi = w.y[i];
        x[i] = fmaf(alpha, pi, x[i]);
        const float ri = fmaf(-alpha, yi, w.r[i]);
        const float zi = ri / diag[i];
        w.r[i] = ri;
        w.z[i] = zi;
        rr += (double)ri * ri;
        rz += (double)ri * zi;
    }
    const double t0 = block_sum(rr, sm);
    const double t1 = block_sum(rz, sm);
    if (threadIdx.x == 0) {
        w.part2[3 * blk] = t0;
        w.part2[3 * blk + 1] = t1;
        w.part2[3 * blk + 2] = t1;      // r.z with z = r / diag everywhere: what a fallback to Jacobi continues with
    }
}

// partial r.z again (second column of part2) after the coarse slice of z changed; init: p = z as well
__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_rz(PcgWork w, int copy_p) {
    SPCG_BLOCK_PROLOGUE(!copy_p)
    if (!copy_p && w.sc[seg].jacobi) return;      // this segment's z is the Jacobi one of k_spcg_update: its partial is in place
    double rz = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += PCG_BLOCK) {
        const float zi = w.z[i];
        if (copy_p) w.p[i] = zi;
        rz += (double)w.r[i] * zi;
    }
    const double t = block_sum(rz, sm);
    if (threadIdx.x == 0) w.part2[3 * blk + 1] = t;
}

// p = z + beta p ; the first block of a segment publishes the scalars of its finished iteration
// Breakdown (r.z <= 0: the Chebyshev polynomial of the coarse-level block lost definiteness -- its eigenvalue bound was too small --
// or the residual ran away): the segment RESTARTS its conjugate gradients from the current x with Jacobi alone, p = z = r / diag,
// r.z from the third column of the partials (k_spcg_update); from then on the Chebyshev kernels skip it (SegScalars.jacobi).
// Every block of the segment takes the same decision from the same reduced numbers -- no flag is read here, so nothing races with
// the first block's write.  With Jacobi already in use the two r.z columns are equal, i.e. r.z <= 0 there is a hard failure.
__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_pupdate(PcgWork w, const float* __restrict__ diag, int parity, float tol) {
    SPCG_BLOCK_PROLOGUE(true)
    const int b0 = w.seg_blk[seg], nb = w.seg_blk[seg + 1] - b0;
    const double rr = reduce_partials(w.part2 + 3 * (int64_t)b0, nb, 3, sm);
    const double rz_new = reduce_partials(w.part2 + 3 * (int64_t)b0 + 1, nb, 3, sm);
    const double rz_jac = reduce_partials(w.part2 + 3 * (int64_t)b0 + 2, nb, 3, sm);
    const double rz_old = w.sc[seg].rz[parity];
    const double bb = w.sc[seg].bb;
    const double rel = sqrt(rr / bb);
    const bool bad = !(rz_new > 0.0) || !(rel < 1e4);
    const bool fall = bad && rz_jac > 0.0 && rz_jac != rz_new && rel < 1e30;
    if (fall) {
        for (int i = lo + threadIdx.x; i < hi; i += PCG_BLOCK) { const float zi = w.r[i] / diag[i]; w.z[i] = zi; w.p[i] = zi; }
    } else {
        const float beta = (float)(rz_new / rz_old);
        for (int i = lo + threadIdx.x; i < hi; i += PCG_BLOCK) w.p[i] = fmaf(beta, w.p[i], w.z[i]);
    }
    __syncthreads();
    if (blk == b0 && threadIdx.x == 0) {
        SegScalars& s = w.sc[seg];
        s.rz[parity ^ 1] = fall ? rz_jac : rz_new;
        s.rel = rel;
        s.iter += 1;
        if (fall) s.jacobi = 1;
        if (rel <= (double)tol) { s.done = 1; seg_retire(w); }
        else if (!fall && (!(rz_new > 0.0) || !(rel < 1e30))) { s.done = 2; seg_retire(w); }      // r.z <= 0 with Jacobi (or NaN): nothing left to fall back to
    }
}

// what the host reads every check_every iterations (+ the per-segment results, when asked for)
__global__ void __launch_bounds__(PCG_BLOCK) k_spcg_summary(PcgWork w, double* __restrict__ seg_info) {
    __shared__ double smr[PCG_BLOCK];
    __shared__ int smi[PCG_BLOCK], smb[PCG_BLOCK], smn[PCG_BLOCK], smf[PCG_BLOCK];
    double mr = 0.0;
    int mi = 0, nbk = 0, mn = 0x7fffffff, nfb = 0;
    for (int c = threadIdx.x; c < w.nseg; c += PCG_BLOCK) {
        const SegScalars& s = w.sc[c];
        mr = s.rel > mr ? s.rel : mr;
        mi = s.iter > mi ? s.iter : mi;
        mn = s.iter < mn ? s.iter : mn;
        nbk += s.done == 2;
        nfb += s.jacobi != 0;
        if (seg_info) { seg_info[2 * c] = (double)s.iter; seg_info[2 * c + 1] = s.done == 2 ? -s.rel : s.rel; }
    }
    smr[threadIdx.x] = mr; smi[threadIdx.x] = mi; smb[threadIdx.x] = nbk; smn[threadIdx.x] = mn; smf[threadIdx.x] = nfb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < PCG_BLOCK; ++t) { mr = smr[t] > mr ? smr[t] : mr; mi = smi[t] > mi ? smi[t] : mi; nbk += smb[t]; mn = smn[t] < mn ? smn[t] : mn; nfb += smf[t]; }
        w.g->max_rel = nbk ? -mr : mr;         // negative: some segment broke down (r.z <= 0)
        w.g->max_iter = mi;
        w.g->min_iter = mn;
        w.g->fallbacks = nfb;
    }
}

// ---- optional live profiling of the operator launches (bench.py's roofline leg) -----------------
static int g_prof_enable = 0;
static double g_prof_ms = 0.0;
static long long g_prof_launches = 0;
static double g_prof_alg_bytes = 0.0, g_prof_phys_bytes = 0.0, g_prof_survey_bytes = 0.0, g_prof_last_survey = 0.0;
// several host threads may run solves at once (chunks on separate streams): every thread times with its own event pool and
// adds to the shared accumulators under a lock
static thread_local std::vector<hipEvent_t> g_prof_events;
static std::mutex g_prof_mutex;
static std::vector<float> g_prof_last_samples;
static std::vector<float> g_prof_samples;      // milliseconds of every timed application since the last nksr_pcg_profile call (at most 65536)

// the bytes of the timed applications (PcgOperator::bytes; the CSR SpMV's: spmv_bytes of csrc/spmv.hip)
extern "C" int nksr_pcg_profile_bytes(double* algorithmic_out, double* physical_out) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if (algorithmic_out) *algorithmic_out = g_prof_alg_bytes;
    if (physical_out) *physical_out = g_prof_phys_bytes;
    g_prof_last_survey = g_prof_survey_bytes;
    g_prof_alg_bytes = g_prof_phys_bytes = g_prof_survey_bytes = 0.0;
    return NKSR_OK;
}
// the same launches priced by SURVEY.md section 8d's formula (the CSR SpMV: identical to the algorithmic figure; the matrix-free
// operator: 16 bytes per stored entry, which it does not move) -- the value of the last nksr_pcg_profile_bytes call
extern "C" double nksr_pcg_profile_survey_bytes(void) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    return g_prof_last_survey;
}

extern "C" int nksr_pcg_profile(int enable, double* ms_out, int64_t* launches_out) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if (ms_out) *ms_out = g_prof_ms;
    if (launches_out) *launches_out = g_prof_launches;
    g_prof_ms = 0.0;
    g_prof_launches = 0;
    g_prof_enable = enable;
    g_prof_last_samples.swap(g_prof_samples);
    g_prof_samples.clear();
    return NKSR_OK;
}
// the individual durations (milliseconds) behind the totals the LAST nksr_pcg_profile call returned: a slow box or a slow launch is
// visible in min / median, not in a mean
extern "C" int64_t nksr_pcg_profile_samples(float* ms_out, int64_t capacity) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    const int64_t n = (int64_t)g_prof_last_samples.size() < capacity ? (int64_t)g_prof_last_samples.size() : capacity;
    for (int64_t i = 0; i < n && ms_out; ++i) ms_out[i] = g_prof_last_samples[i];
    return (int64_t)g_prof_last_samples.size();
}

int nksr_pcg_run(PcgOperator& A, const float* diag, int32_t M, const float* b, float* x, float tol, int max_iter, int check_every,
                 void* vector_workspace, double* info_out, hipStream_t st, const nksr_coarse_precond_t* pc, const nksr_segments_t* seg) {
    if (M <= 0) { if (info_out) { info_out[0] = 0; info_out[1] = 0; info_out[2] = 0; } return NKSR_OK; }
    if (!vector_workspace) return nksr_set_error(NKSR_ERR_ARG, "workspace is NULL");
    if (seg && (seg->nseg < 1 || seg->nranges < 1 || !seg->lo || !seg->hi)) return nksr_set_error(NKSR_ERR_ARG, "bad segments");
    if (check_every < 1) check_every = 1;
    PcgWork w = carve(vector_workspace, M, seg);
    const dim3 gb(w.nb_max), blkd(PCG_BLOCK);
    if (pc) {
        if (int rc = cheb_check(pc, w.nseg)) return rc;
        if (pc->first < 0 || pc->first + pc->n != M) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner: the block must be the last %d unknowns", pc->n);
        cheb_coeffs(pc, w.nseg, st);
    }
    hipLaunchKernelGGL(k_seg_count, dim3(nksr_blocks(w.nseg, 64)), dim3(64), 0, st, w);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(1), 0, st, w);
    hipLaunchKernelGGL(k_seg_fill, dim3(nksr_blocks((int64_t)w.nseg * w.nranges * 64, 256)), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_spcg_init, gb, blkd, 0, st, w, b, diag, x);
    if (pc) {
        cheb_apply(pc, w.r + pc->first, w.z + pc->first, nullptr, st);
        hipLaunchKernelGGL(k_spcg_rz, gb, blkd, 0, st, w, 1);
    }
    hipLaunchKernelGGL(k_spcg_init_finish, dim3(w.nseg), blkd, 0, st, w, diag);
    NKSR_CHECK_LAUNCH();
    PcgGlobal host;
    memset(&host, 0, sizeof(host));
    int launched = 0;
    const bool prof = g_prof_enable != 0;
    if (prof)
        while ((int)g_prof_events.size() < 2 * check_every) {
            hipEvent_t e;
            NKSR_CHECK_HIP(hipEventCreate(&e));
            g_prof_events.push_back(e);
        }
    // (Tried in round 3 and removed: capturing two iterations into a hipGraph and replaying it for small systems -- configs[1] and the
    // 10 000-point bunny sequence spend 5 / 8 ms in 42 / 93 iterations of 6-20 tiny launches.  No change (5.07 vs 4.56 ms, 8.76 vs 8.30):
    // the bound is the dependency latency between consecutive tiny kernels on the device, ~15 us each, not the host enqueue.)
    auto iterate = [&](int parity, int c) -> int {
        if (prof) (void)hipEventRecord(g_prof_events[2 * c], st);
        if (int rc = A.apply(w.p, w.y, &w.g->done_all, w.nseg > 1 ? &w.sc[0].done : nullptr, (int)(sizeof(SegScalars) / sizeof(int)), &w.g->done_count, w.nseg, st)) return rc;
        if (prof) (void)hipEventRecord(g_prof_events[2 * c + 1], st);
        hipLaunchKernelGGL(k_spcg_dot, gb, blkd, 0, st, w);
        hipLaunchKernelGGL(k_spcg_update, gb, blkd, 0, st, w, diag, x, parity);
        if (pc) {
            cheb_apply(pc, w.r + pc->first, w.z + pc->first, w.sc, st);
            hipLaunchKernelGGL(k_spcg_rz, gb, blkd, 0, st, w, 0);
        }
        hipLaunchKernelGGL(k_spcg_pupdate, gb, blkd, 0, st, w, diag, parity, tol);
        return NKSR_OK;
    };
    while (launched < max_iter) {
        int chunk = check_every < (max_iter - launched) ? check_every : (max_iter - launched);
        for (int c = 0; c < chunk; ++c)
            if (int rc = iterate((launched + c) & 1, c)) return rc;
        hipLaunchKernelGGL(k_spcg_summary, dim3(1), blkd, 0, st, w, seg ? seg->info : (double*)nullptr);
        NKSR_CHECK_LAUNCH();
        NKSR_CHECK_HIP(hipMemcpyAsync(&host, w.g, sizeof(host), hipMemcpyDeviceToHost, st));
        NKSR_CHECK_HIP(hipStreamSynchronize(st));
        if (prof) {
            // only applications in which EVERY segment was still iterating (the done flag turns later launches into no-ops, and the
            // operator skips the rows of segments that have converged: those move fewer bytes than A.bytes() says)
            double ba, bp, bs;
            A.bytes(&ba, &bp, &bs);
            std::lock_guard<std::mutex> lock(g_prof_mutex);
            for (int c = 0; c < chunk && launched + c < host.min_iter; ++c) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, g_prof_events[2 * c], g_prof_events[2 * c + 1]) == hipSuccess) {
                    g_prof_ms += ms;
                    g_prof_launches += 1;
                    if (g_prof_samples.size() < 65536) g_prof_samples.push_back(ms);
                    g_prof_alg_bytes += ba;
                    g_prof_phys_bytes += bp;
                    g_prof_survey_bytes += bs;
                }
            }
        }
        launched += chunk;
        if (host.done_all) break;
    }
    if (info_out) {
        info_out[0] = (double)host.max_iter;
        info_out[1] = host.max_rel;          // negative: a segment stopped on r.z <= 0 with Jacobi too, or on NaN (hard failure)
        info_out[2] = (double)host.fallbacks; // segments whose coarse-level block lost definiteness: they went on with Jacobi alone
    }
    return NKSR_OK;
}

struct CsrOperator : PcgOperator {
    const int32_t* rowptr; const void* cols; const float* vals; int M; int64_t nnz; int fmt; SpmvPlan plan;
    int apply(const float* p, float* y, const int* done, const int*, int, const int*, int, hipStream_t st) override {
        launch_spmv(rowptr, cols, vals, M, nnz, fmt, plan, p, y, done, st);
        return NKSR_OK;
    }
    void bytes(double* a, double* ph, double* sv) override { spmv_bytes(M, nnz, fmt, a, ph); *sv = *a; }
};

extern "C" int nksr_pcg_solve(const int32_t* rowptr, const void* cols, const float* vals, const float* diag, int32_t M,
                              int64_t nnz, int col_format, const float* b, float* x, float tol, int max_iter, int check_every,
                              void* workspace, const nksr_coarse_precond_t* pc, double* info_out, void* stream) {
    if (M <= 0) { if (info_out) { info_out[0] = 0; info_out[1] = 0; info_out[2] = 0; } return NKSR_OK; }
    if (!workspace) return nksr_set_error(NKSR_ERR_ARG, "workspace is NULL");
    void* spmv_ws = (char*)workspace + pcg_vector_bytes(M);
    int rc = nksr_spmv_plan(rowptr, M, nnz, col_format, spmv_ws, stream);
    if (rc) return rc;
    CsrOperator A;
    A.rowptr = rowptr; A.cols = cols; A.vals = vals; A.M = M; A.nnz = nnz; A.fmt = col_format;
    A.plan = carve_spmv(spmv_ws, nnz, col_format);
    return nksr_pcg_run(A, diag, M, b, x, tol, max_iter, check_every, workspace, info_out, (hipStream_t)stream, pc);
}
