// ---- coarse-level block preconditioner -------------------------------------------------------------------------------------------
// The multi-level system is badly conditioned through its COARSE basis functions (each overlaps 124 neighbours of its own level and
// every finer voxel under its support): Jacobi needs 47 iterations per tree_depth-5 chunk where an exact solve of the diagonal
// block of the levels >= 2 (8 % of the unknowns, 4.5 % of the non-zeros) would need 12.  That block A_cc is assembled once per
// solve (plain CSR, nksr_assemble on the hierarchy with its fine levels masked) and z_c ~ A_cc^-1 r_c is approximated by a FIXED
// number of Jacobi-preconditioned Chebyshev steps -- a fixed polynomial in A_cc, hence a constant SPD preconditioner (plain CG
// stays valid) and deterministic.  One kernel per step, one wavefront per row:
//   t = (A_cc d)_j;  y_j += d_j;  res_j -= t;  d'_j = a d_j + b res_j / D_j          (d double-buffered: rows read their neighbours' d)
// Batched chunk solves: A_cc is block diagonal, every segment has its own eigenvalue bound and therefore its own polynomial
// (coefficient table coef[segment][1 + 2 i], row_seg = segment of every coarse row).
// The conjugate-gradient loop (csrc/pcg.hip) reaches this file through cheb.h; of the loop's state the kernels here see only
// seg_skipped (csrc/pcg_dev.h).
#include "common.h"
#include "pcg_dev.h"
#include "cheb.h"
#include "coarse_pack_dev.h"

#define CHEB_STRIDE (1 + 2 * NKSR_PC_MAX_STEPS)

// coef[c] = { 1 / theta, a_0, b_0, a_1, b_1, ... } for the interval [lmax / ratio, lmax], lmax = scale * lambda[c]; a segment without
// a usable bound (no constraint rows on its coarse levels) gets { 1, 0, 0, ... }: one Jacobi step
// gersh (may be NULL): a Gershgorin bound of the same spectrum (nksr_coarse_gershgorin) -- a true upper bound, so the margin on the
// power estimate never has to carry the interval beyond it
__global__ void k_cheb_coeffs(int nseg, const float* __restrict__ lambda, const float* __restrict__ gersh, float scale, float ratio, int steps,
                              float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nseg) return;
    float* o = coef + (int64_t)c * CHEB_STRIDE;
    double lmax = (double)scale * (double)lambda[c];
    if (gersh && gersh[c] > 0.f && (double)gersh[c] < lmax) lmax = (double)gersh[c];
    if (!(lmax > 0.0) || !(lmax < 1e30)) {
        o[0] = 1.f;
        for (int i = 0; i < steps; ++i) { o[1 + 2 * i] = 0.f; o[2 + 2 * i] = 0.f; }
        return;
    }
    const double lmin = lmax / (double)ratio, theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    double rho = 1.0 / sigma;
    o[0] = (float)(1.0 / theta);
    for (int i = 0; i < steps; ++i) {
        const double rho_n = 1.0 / (2.0 * sigma - rho);
        o[1 + 2 * i] = (float)(rho_n * rho);
        o[2 + 2 * i] = (float)(2.0 * rho_n / delta);
        rho = rho_n;
    }
}

__global__ void __launch_bounds__(256) k_cheb_init(int n, const float* __restrict__ r, const float* __restrict__ diag,
                                                   const float* __restrict__ coef, const int32_t* __restrict__ row_seg,
                                                   float* __restrict__ res, float* __restrict__ d0, float* __restrict__ y,
                                                   const SegScalars* __restrict__ sc) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int seg = row_seg ? row_seg[j] : 0;
    if (seg_skipped(sc, seg)) return;
    const float rj = r[j];
    res[j] = rj;
    d0[j] = rj / diag[j] * (coef ? coef[(int64_t)seg * CHEB_STRIDE] : 1.f);
    y[j] = 0.f;
}

// (A v)_j of a CSR row by one wavefront, the sum in every lane.  A wavefront's time is a chain of dependent load latencies (the block
// streams from L2 / HBM): four 64-entry groups (rows hold ~190 entries) are in flight at once -- clamped addresses instead of
// predicated loads, so that the compiler does not serialise them.  Fixed order: group sums (t0 + t1) + (t2 + t3), then the butterfly.
__device__ __forceinline__ float csr_row_dot(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                             const float* __restrict__ vals, int j, int lane, const float* __restrict__ v) {
    const int k0 = rowptr[j], k1 = rowptr[j + 1];
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int base = k0 + lane; base - lane < k1; base += 256) {
        float a[4];
        int c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = base + 64 * q, kc = k < k1 ? k : k1 - 1;
            a[q] = vals[kc];
            c[q] = cols[kc];
            if (k >= k1) a[q] = 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = fmaf(a[q], v[c[q]], t[q]);
    }
    float tt = (t[0] + t[1]) + (t[2] + t[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tt += __shfl_xor(tt, o);
    return tt;
}

__global__ void __launch_bounds__(256) k_cheb_step(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                   const float* __restrict__ vals, const float* __restrict__ diag,
                                                   const float* __restrict__ coef, int step, const int32_t* __restrict__ row_seg,
                                                   float* __restrict__ res, const float* __restrict__ d_old, float* __restrict__ d_new,
                                                   float* __restrict__ y, const SegScalars* __restrict__ sc) {
    const int j = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (j >= n) return;
    const int seg = row_seg ? row_seg[j] : 0;
    if (seg_skipped(sc, seg)) return;
    // everything that does not depend on the row's entries is requested up front, with the row pointers
    const float dj = d_old[j], rs = res[j], dg = diag[j], yj = y[j];
    const float a = coef[(int64_t)seg * CHEB_STRIDE + 1 + 2 * step], b = coef[(int64_t)seg * CHEB_STRIDE + 2 + 2 * step];
    const float tt = csr_row_dot(rowptr, cols, vals, j, lane, d_old);
    if (lane == 0) {
        const float rj = rs - tt;
        y[j] = yj + dj;
        res[j] = rj;
        d_new[j] = fmaf(a, dj, b * rj / dg);
    }
}

// v' = D^-1 A_cc v (power iteration for the largest eigenvalue of the Jacobi-scaled block)
__global__ void __launch_bounds__(256) k_coarse_power(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                      const float* __restrict__ vals, const float* __restrict__ diag,
                                                      const float* __restrict__ v, float* __restrict__ out) {
    const int j = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (j >= n) return;
    const float dg = diag[j];
    const float t = csr_row_dot(rowptr, cols, vals, j, lane, v);
    if (lane == 0) out[j] = t / dg;
}

__global__ void __launch_bounds__(256) k_fill1(int n, float* __restrict__ v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = 1.f;
}

// out[blockIdx.x] = sqrt(sum b^2 / sum a^2) = ||b|| / ||a|| over the rows of this workgroup's segment: its ranges in order, fixed
// strides (segment-relative order).  range(k, l, h): the k-th range [l, h) of the segment, false to pass it over.
template <typename Range>
__device__ __forceinline__ void norm_ratio(int nranges, Range range, const float* __restrict__ a, const float* __restrict__ b,
                                           float* __restrict__ out) {
    __shared__ double sm[PCG_BLOCK / 64];
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < nranges; ++k) {
        int l, h;
        if (!range(k, l, h)) continue;
        for (int i = l + threadIdx.x; i < h; i += PCG_BLOCK) { sa += (double)a[i] * a[i]; sb += (double)b[i] * b[i]; }
    }
    const double ta = block_sum(sa, sm), tb = block_sum(sb, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = ta > 0.0 ? (float)sqrt(tb / ta) : 0.f;
}
// one workgroup per segment c: the coarse rows of its ranges lo / hi (unknown numbers; the block starts at `first`).  Without
// segments: the whole block.
__global__ void __launch_bounds__(PCG_BLOCK) k_norm_ratio(int n, int first, int nranges, const int32_t* __restrict__ lo,
                                                          const int32_t* __restrict__ hi, const float* __restrict__ a,
                                                          const float* __restrict__ b, float* __restrict__ out) {
    const int c = blockIdx.x;
    norm_ratio(nranges, [&](int k, int& l, int& h) {
        l = lo ? lo[c * nranges + k] - first : 0; h = lo ? hi[c * nranges + k] - first : n;
        if (h > n) h = n;
        if (l < 0) { if (h <= 0) return false; l = 0; }       // ranges of the fine levels lie below `first`
        return true;
    }, a, b, out);
}
// the rows [seg_base[c], seg_base[c + 1]) (segment-major order): the single range of segment c
__global__ void __launch_bounds__(PCG_BLOCK) k_norm_ratio_seg(const int32_t* __restrict__ seg_base, const float* __restrict__ a,
                                                              const float* __restrict__ b, float* __restrict__ out) {
    const int c = blockIdx.x;
    norm_ratio(1, [&](int, int& l, int& h) { l = seg_base[c]; h = seg_base[c + 1]; return true; }, a, b, out);
}

extern "C" int nksr_coarse_lambda_max(const int32_t* rowptr, const int32_t* cols, const float* vals, const float* diag, int32_t n, int iters,
                                      float* work, float* lambda_out, const nksr_segments_t* seg, int32_t first, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!rowptr || !cols || !vals || !diag || !work || !lambda_out) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    if (seg && (seg->nseg < 1 || seg->nranges < 1 || !seg->lo || !seg->hi)) return nksr_set_error(NKSR_ERR_ARG, "bad segments");
    if (iters < 2) iters = 2;
    hipStream_t st = (hipStream_t)stream;
    float* v[2] = {work, work + n};
    const dim3 g1(nksr_blocks(n, 256)), gw(nksr_blocks((int64_t)n * 64, 256));
    hipLaunchKernelGGL(k_fill1, g1, dim3(256), 0, st, n, v[0]);
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(k_coarse_power, gw, dim3(256), 0, st, n, rowptr, cols, vals, diag, (const float*)v[i & 1], v[(i + 1) & 1]);
    hipLaunchKernelGGL(k_norm_ratio, dim3(seg ? seg->nseg : 1), dim3(PCG_BLOCK), 0, st, n, seg ? first : 0, seg ? seg->nranges : 1,
                       seg ? seg->lo : (const int32_t*)nullptr, seg ? seg->hi : (const int32_t*)nullptr, (const float*)v[(iters - 1) & 1],
                       (const float*)v[iters & 1], lambda_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// ---- packed coarse block (nksr_coarse_precond_t.format 1) -----------------------------------------------------------------------
// A Chebyshev step streams the whole block: 8 bytes per entry (fp32 value + int32 column) x 4.2e8 entries x 8 steps per PCG
// iteration on the 64-chunk scene -- a third of the iteration.  The preconditioner only has to be a FIXED symmetric positive
// operator, so the block is stored Jacobi-scaled, S = D^-1/2 A_cc D^-1/2 (unit diagonal, |S_ij| <= 1): an entry is a 16-bit
// half-precision value and a 16-bit column LOCAL to the row's segment -- the coarse unknowns are renumbered segment-major
// (old_of_new), so a chunk's columns span < 2^16 -- i.e. 4 bytes.  The recurrence runs in the scaled variables
//   res' = D^-1/2 res,  d' = D^1/2 d:   t = S d';  y' += d';  res' -= t;  d' <- a d' + b res';      z = D^-1/2 y'
// (the same polynomial in D^-1 A_cc, up to the rounding of S to half precision: S_ij = half(v_ij * (dis_i * dis_j)) is bitwise symmetric).
// The drop rule and the entry word: coarse_pack_dev.h.

__global__ void __launch_bounds__(256) k_cc_count(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                  const float* __restrict__ vals, const float* __restrict__ diag,
                                                  const int32_t* __restrict__ old_of_new, float drop, int32_t* __restrict__ lens) {
    const int i = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (i >= n) return;
    const int j = old_of_new[i];
    const int k0 = rowptr[j], k1 = rowptr[j + 1] - 1;
    const float di = 1.f / sqrtf(diag[j]);
    int cnt = 0;
    for (int k = k0 + lane; k < k1; k += 64) cnt += cc_keep(cc_scaled(vals[k], di, 1.f / sqrtf(diag[cols[k]])), drop) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) lens[i] = cnt;
}

__global__ void __launch_bounds__(256) k_cc_pack(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                 const float* __restrict__ vals, const float* __restrict__ diag,
                                                 const int32_t* __restrict__ old_of_new, const int32_t* __restrict__ new_of_old,
                                                 const int32_t* __restrict__ row_seg, const int32_t* __restrict__ seg_base,
                                                 const int32_t* __restrict__ prow, float drop, uint32_t* __restrict__ pk, float* __restrict__ dis) {
    const int i = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (i >= n) return;
    const int j = old_of_new[i];
    const int k0 = rowptr[j], k1 = rowptr[j + 1] - 1;          // the diagonal closes every row: it is dropped (unit diagonal)
    const float di = 1.f / sqrtf(diag[j]);
    const int base = seg_base[row_seg[i]];
    int o = prow[i];
    if (lane == 0) dis[i] = di;
    for (int kb = k0; kb < k1; kb += 64) {                      // kept entries keep their order
        const int k = kb + lane;
        bool keep = false;
        uint32_t word = 0u;
        if (k < k1) {
            const int c = cols[k];
            const __half hv = cc_scaled(vals[k], di, 1.f / sqrtf(diag[c]));
            keep = cc_keep(hv, drop);
            word = cc_word(hv, (uint32_t)(new_of_old[c] - base));
        }
        const unsigned long long m = __ballot(keep);
        if (keep) pk[o + __popcll(m & ((1ull << lane) - 1ull))] = word;
        o += __popcll(m);
    }
}

__global__ void __launch_bounds__(256) k_cheb16_init(int n, const float* __restrict__ r, const int32_t* __restrict__ old_of_new,
                                                     const float* __restrict__ dis, const float* __restrict__ coef,
                                                     const int32_t* __restrict__ row_seg, float* __restrict__ res, float* __restrict__ d0,
                                                     float* __restrict__ y, const SegScalars* __restrict__ sc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int seg = row_seg[i];
    if (seg_skipped(sc, seg)) return;
    const float rs = r[old_of_new[i]] * dis[i];
    res[i] = rs;
    d0[i] = rs * (coef ? coef[(int64_t)seg * CHEB_STRIDE] : 1.f);
    y[i] = 0.f;
}

// One wavefront per CHEB16_ROWS = 16 consecutive rows, 16 lanes per row: lane (g, l) = (lane >> 4, lane & 15) works for the four rows
// i0 + 4 g + r, r < 4, and takes entries l, l + 16, ... of each.  LAST: the step also leaves z = D^-1/2 (y' + d') in the PCG's order.
// POWER: out = S v only (eigenvalue bound).
// Round 6.  After the drop (entries below 0.5 % of the unit diagonal) a row of the 64-chunk scene keeps 37 entries on average (median
// 28, a tenth none, 1 % more than 300: tools/cheb_rows_probe.py), not the ~240 it is assembled with.  Rounds 3-5 gave every row one
// 256-entry trip of a whole wavefront (four rows per wavefront: 16 entry loads + 16 gathers, ~85 % of their lanes clamped and masked)
// and ran at the latency of row pointers -> entries -> gathered vector over 380 000 wavefronts per step.  Sixteen lanes per row put
// the same 16 + 16 loads in flight for FOUR times the rows -- a row's partial sums depend on its own length only, so its result does
// not depend on its wave mates (a chunk alone == the chunk in a batch).
#define CHEB16_ROWS 16
template <bool POWER>
__global__ void __launch_bounds__(256) k_cheb16_step(int n, const int32_t* __restrict__ prow, const uint32_t* __restrict__ pk,
                                                     const float* __restrict__ coef, int step, const int32_t* __restrict__ row_seg,
                                                     const int32_t* __restrict__ seg_base, float* __restrict__ res,
                                                     const float* __restrict__ d_old, float* __restrict__ d_new, float* __restrict__ y,
                                                     const SegScalars* __restrict__ sc, int last, float* __restrict__ z,
                                                     const int32_t* __restrict__ old_of_new, const float* __restrict__ dis) {
    const int i0 = ((blockIdx.x * 256 + threadIdx.x) >> 6) * CHEB16_ROWS, lane = threadIdx.x & 63;
    if (i0 >= n) return;
    const int g = lane >> 4, l = lane & 15;
    // per-row scalars: lane q (< 16) owns row i0 + q; the row pointers come as one load of 17 lanes
    const int ir = i0 + (lane < CHEB16_ROWS ? lane : 0), irc = ir < n ? ir : n - 1;
    const int pl = prow[(i0 + lane <= n && lane <= CHEB16_ROWS) ? i0 + lane : n];
    const int sg = row_seg[irc];
    const bool live_l = lane < CHEB16_ROWS && ir < n && (POWER || !seg_skipped(sc, sg));
    const int sb = seg_base[sg];
    const float dj = d_old[irc];
    float rs = 0.f, yj = 0.f, ca = 0.f, cb = 0.f;
    if (!POWER) {
        rs = res[irc]; yj = y[irc];
        ca = coef[(int64_t)sg * CHEB_STRIDE + 1 + 2 * step]; cb = coef[(int64_t)sg * CHEB_STRIDE + 2 + 2 * step];
    }
    // the four rows of this lane's group: first / last entry, vector base of their segment (a dead row is empty)
    int k0[4], k1[4], base_r[4];
    int maxlen = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = 4 * g + r;
        k0[r] = __shfl(pl, q);
        k1[r] = __shfl(pl, q + 1);
        base_r[r] = __shfl(sb, q);
        if (!__shfl((int)live_l, q)) k1[r] = k0[r];
        maxlen = (k1[r] - k0[r]) > maxlen ? (k1[r] - k0[r]) : maxlen;
    }
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1) { const int m = __shfl_xor(maxlen, o); maxlen = m > maxlen ? m : maxlen; }     // (over the four groups: one trip count per wavefront)
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < maxlen; b += 64) {                     // four 16-entry trips of every row at once: 16 loads, then 16 gathers
        uint32_t w[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0[r] + b + 16 * q + l;
                const int kc = k < k1[r] ? k : (k1[r] > k0[r] ? k1[r] - 1 : 0);          // clamped address, value masked below
                w[q][r] = pk[kc];
                if (k >= k1[r]) w[q][r] = 0u;                                              // value +0.0, column 0 of the segment
            }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                t[r] = fmaf(cc_word_value(w[q][r]), d_old[base_r[r] + cc_word_col(w[q][r])], t[r]);
    }
    // the 16 lanes of a group sum every row (fixed tree); lane q of the wavefront ends up with the sum of row q
    float tot = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float tt = t[r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) tt += __shfl_xor(tt, o);
        const float got = __shfl(tt, 16 * (lane >> 2) + 0);   // row q = 4 g' + r lives in group g' = q >> 2: lane 16 g' holds its sum
        if (lane < CHEB16_ROWS && (lane & 3) == r) tot = got;
    }
    if (live_l) {
        tot += dj;                                                        // the unit diagonal
        if (POWER) { d_new[ir] = tot; return; }
        const float rj = rs - tot;
        res[ir] = rj;
        d_new[ir] = fmaf(ca, dj, cb * rj);
        if (last) z[old_of_new[ir]] = (yj + dj) * dis[ir];
        else y[ir] = yj + dj;
    }
}
static dim3 cheb16_grid(int n) { return dim3(nksr_blocks(((int64_t)n + CHEB16_ROWS - 1) / CHEB16_ROWS * 64, 256)); }

extern "C" int nksr_coarse_pack_count(const int32_t* rowptr, const int32_t* cols, const float* vals, const float* diag, int32_t n,
                                      const int32_t* old_of_new, float drop_tol, int32_t* lens_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!rowptr || !cols || !vals || !diag || !old_of_new || !lens_out) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    if (!(drop_tol >= 0.f) || drop_tol >= 1.f) return nksr_set_error(NKSR_ERR_ARG, "drop_tol must be in [0, 1)");
    hipLaunchKernelGGL(k_cc_count, dim3(nksr_blocks((int64_t)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, n, rowptr, cols, vals, diag, old_of_new,
                       drop_tol, lens_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_coarse_pack(const int32_t* rowptr, const int32_t* cols, const float* vals, const float* diag, int32_t n,
                                const int32_t* old_of_new, const int32_t* new_of_old, const int32_t* row_seg_new, const int32_t* seg_base,
                                const int32_t* packed_rowptr, float drop_tol, uint32_t* packed_out, float* dis_out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!rowptr || !cols || !vals || !diag || !old_of_new || !new_of_old || !row_seg_new || !seg_base || !packed_rowptr || !packed_out || !dis_out)
        return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    if (!(drop_tol >= 0.f) || drop_tol >= 1.f) return nksr_set_error(NKSR_ERR_ARG, "drop_tol must be in [0, 1)");
    hipLaunchKernelGGL(k_cc_pack, dim3(nksr_blocks((int64_t)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, n, rowptr, cols, vals, diag,
                       old_of_new, new_of_old, row_seg_new, seg_base, packed_rowptr, drop_tol, packed_out, dis_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_coarse_lambda_max_packed(const nksr_coarse_precond_t* pc, int32_t nseg, int iters, float* work, float* lambda_out, void* stream) {
    if (!pc || pc->n <= 0) return NKSR_OK;
    if (pc->format != 1 || !pc->packed || !pc->packed_rowptr || !pc->row_seg || !pc->seg_base || !work || !lambda_out)
        return nksr_set_error(NKSR_ERR_ARG, "packed coarse block has NULL arrays");
    if (iters < 2) iters = 2;
    hipStream_t st = (hipStream_t)stream;
    const int n = pc->n;
    float* v[2] = {work, work + n};
    hipLaunchKernelGGL(k_fill1, dim3(nksr_blocks(n, 256)), dim3(256), 0, st, n, v[0]);
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL((k_cheb16_step<true>), cheb16_grid(n), dim3(256), 0, st, n, pc->packed_rowptr, pc->packed,
                           (const float*)nullptr, 0, pc->row_seg, pc->seg_base, (float*)nullptr, (const float*)v[i & 1], v[(i + 1) & 1], (float*)nullptr,
                           (const SegScalars*)nullptr, 0, (float*)nullptr, (const int32_t*)nullptr, (const float*)nullptr);
    hipLaunchKernelGGL(k_norm_ratio_seg, dim3(nseg), dim3(PCG_BLOCK), 0, st, pc->seg_base, (const float*)v[(iters - 1) & 1], (const float*)v[iters & 1], lambda_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

// Gershgorin bound of the Jacobi-scaled block per segment: max over the rows of  sum_j |a_ij| / d_i  (format 0, spectrum of D^-1 A_cc)
// or  1 + sum_j |S_ij|  (format 1: unit diagonal).  2-3x above the true lambda_max on these blocks -- too loose to BE the interval
// (it costs ~50 % more iterations), right as a cap on margin x power estimate.
__global__ void __launch_bounds__(256) k_gersh_rows(int n, int format, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                    const float* __restrict__ vals, const float* __restrict__ diag,
                                                    const uint32_t* __restrict__ pk, float* __restrict__ rowsum) {
    const int i = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (i >= n) return;
    const int k0 = rowptr[i], k1 = rowptr[i + 1];
    float t = 0.f;
    if (format == 1) {
        for (int k = k0 + lane; k < k1; k += 64) t += fabsf(cc_word_value(pk[k]));
    } else {
        for (int k = k0 + lane; k < k1; k += 64) t += fabsf(vals[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) rowsum[i] = format == 1 ? 1.f + t : t / diag[i];
}
__global__ void __launch_bounds__(PCG_BLOCK) k_gersh_seg(int n, const int32_t* __restrict__ seg_base, const int32_t* __restrict__ row_seg,
                                                         int nseg, const float* __restrict__ rowsum, float* __restrict__ out) {
    __shared__ float sm[PCG_BLOCK];
    const int c = blockIdx.x;
    float m = 0.f;
    if (seg_base) {
        for (int i = seg_base[c] + threadIdx.x; i < seg_base[c + 1]; i += PCG_BLOCK) m = fmaxf(m, rowsum[i]);
    } else {
        for (int i = threadIdx.x; i < n; i += PCG_BLOCK)
            if (nseg == 1 || !row_seg || row_seg[i] == c) m = fmaxf(m, rowsum[i]);
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int o = PCG_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = sm[0];
}
extern "C" int nksr_coarse_gershgorin(const nksr_coarse_precond_t* pc, int32_t nseg, float* work, float* gersh_out, void* stream) {
    if (!pc || pc->n <= 0) return NKSR_OK;
    if (!work || !gersh_out || nseg < 1) return nksr_set_error(NKSR_ERR_ARG, "NULL arrays");
    if (pc->format == 1 ? (!pc->packed || !pc->packed_rowptr || !pc->seg_base) : (!pc->rowptr || !pc->vals || !pc->diag || (nseg > 1 && !pc->row_seg)))
        return nksr_set_error(NKSR_ERR_ARG, "coarse block has NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    const int n = pc->n;
    hipLaunchKernelGGL(k_gersh_rows, dim3(nksr_blocks((int64_t)n * 64, 256)), dim3(256), 0, st, n, pc->format, pc->format == 1 ? pc->packed_rowptr : pc->rowptr,
                       pc->cols, pc->vals, pc->diag, pc->packed, work);
    hipLaunchKernelGGL(k_gersh_seg, dim3(nseg), dim3(PCG_BLOCK), 0, st, n, pc->format == 1 ? pc->seg_base : (const int32_t*)nullptr, pc->row_seg, nseg,
                       (const float*)work, gersh_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

int cheb_check(const nksr_coarse_precond_t* pc, int nseg) {
    if (pc->n <= 0 || pc->steps < 1 || pc->steps > NKSR_PC_MAX_STEPS) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner: 1..%d steps", NKSR_PC_MAX_STEPS);
    if (!(pc->lambda_scale > 0.f) || !(pc->ratio > 1.f)) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner: lambda_scale > 0, ratio > 1");
    if (!pc->work || !pc->lambda || !pc->coef) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner has NULL arrays");
    if (pc->format == 1) {
        if (!pc->packed || !pc->packed_rowptr || !pc->dis || !pc->old_of_new || !pc->seg_base || !pc->row_seg)
            return nksr_set_error(NKSR_ERR_ARG, "packed coarse block has NULL arrays");
        return NKSR_OK;
    }
    if (!pc->rowptr || !pc->cols || !pc->vals || !pc->diag) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner has NULL arrays");
    if (nseg > 1 && !pc->row_seg) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner: row_seg is required with more than one segment");
    return NKSR_OK;
}
void cheb_coeffs(const nksr_coarse_precond_t* pc, int nseg, hipStream_t st) {
    hipLaunchKernelGGL(k_cheb_coeffs, dim3(nksr_blocks(nseg, 64)), dim3(64), 0, st, nseg, pc->lambda, pc->gersh, pc->lambda_scale, pc->ratio, pc->steps, pc->coef);
}
// z_c = p_k(A_cc) r_c  (r, z: the coarse slices of the PCG vectors)
void cheb_apply(const nksr_coarse_precond_t* pc, const float* r, float* z, const SegScalars* sc, hipStream_t st) {
    const int n = pc->n;
    float *res = pc->work, *d[2] = {pc->work + n, pc->work + 2 * (size_t)n};
    if (pc->format == 1) {      // packed block: scaled variables, segment-major order; y lives in the work array (z is written by the last step)
        float* y = pc->work + 3 * (size_t)n;
        hipLaunchKernelGGL(k_cheb16_init, dim3(nksr_blocks(n, 256)), dim3(256), 0, st, n, r, pc->old_of_new, pc->dis, (const float*)pc->coef, pc->row_seg,
                           res, d[0], y, sc);
        for (int i = 0; i < pc->steps; ++i)
            hipLaunchKernelGGL((k_cheb16_step<false>), cheb16_grid(n), dim3(256), 0, st, n, pc->packed_rowptr, pc->packed,
                               (const float*)pc->coef, i, pc->row_seg, pc->seg_base, res, (const float*)d[i & 1], d[(i + 1) & 1], y, sc,
                               i == pc->steps - 1 ? 1 : 0, z, pc->old_of_new, pc->dis);
        return;
    }
    hipLaunchKernelGGL(k_cheb_init, dim3(nksr_blocks(n, 256)), dim3(256), 0, st, n, r, pc->diag, (const float*)pc->coef, pc->row_seg, res, d[0], z, sc);
    for (int i = 0; i < pc->steps; ++i)
        hipLaunchKernelGGL(k_cheb_step, dim3(nksr_blocks((int64_t)n * 64, 256)), dim3(256), 0, st, n, pc->rowptr, pc->cols, pc->vals, pc->diag,
                           (const float*)pc->coef, i, pc->row_seg, res, (const float*)d[i & 1], d[(i + 1) & 1], z, sc);
}
// the operator by itself, as the solve applies it to its first residual: the checks, the coefficient table, one application
extern "C" int nksr_coarse_precond_apply(const nksr_coarse_precond_t* pc, int32_t nseg, const float* r, float* z, void* stream) {
    if (!pc) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner is NULL");
    if (nseg < 1) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner: nseg must be >= 1");
    if (int rc = cheb_check(pc, nseg)) return rc;
    if (!r || !z) return nksr_set_error(NKSR_ERR_ARG, "coarse preconditioner: r / z is NULL");
    hipStream_t st = (hipStream_t)stream;
    cheb_coeffs(pc, nseg, st);
    cheb_apply(pc, r, z, nullptr, st);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
