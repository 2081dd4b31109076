// Fast Point Feature Histograms (Rusu 2009; nksr_amd/global_register.py: cloud.compute_fpfh_feature).  include/nksr_hip.h states
// the definition -- which neighbours take part, the pair features in fp64 without fused multiply-adds, the bins -- and the two
// kernels are held to it:
//
//   k_spfh   nksr_spfh: ONE LANE PER POINT walks the point's k <= 32 neighbours (idx / d2 as the kNN query wrote them), forms the
//            three angular features of every participating pair and counts them into 3 x 11 bins.  The histogram of a lane is 33
//            counters indexed by a value the lane computes, and a per-lane int[33] indexed that way goes to scratch memory; counts
//            are <= 32, so a lane keeps them as 33 BYTES of LDS instead (a row of 36: 9 dwords, an odd stride, so the 64 lanes of a
//            wavefront start in 64 different banks).  The other choice -- a group of lanes per point -- would need the counters
//            shared and bumped atomically; one lane per point needs no atomics and the pair arithmetic (fp64, an atan2) is what
//            costs, not the 32 loads per lane.  The rows leave through the block: 256 x 33 consecutive ints, coalesced.
//   k_fpfh   nksr_fpfh: ONE LANE PER (point, bin), 33 lanes per point, FPFH_POINTS points per workgroup.  The lane adds the weighted
//            SPFH of the participating neighbours in ascending neighbour order (the 33 lanes of a point read 33 consecutive counts of
//            one neighbour row), F goes to LDS, and every lane sums the 11 values of its third from there in ascending bin order --
//            the same sequence in all 11 lanes of a third, so they scale by the same bits.
// Integers (k_spfh) and sums in an order fixed by the inputs alone (k_fpfh): no atomics, the same call gives the same bits.
#include "common.h"

#define SPFH_BLOCK 256
#define SPFH_ROW 36                 // bytes of LDS per lane: 33 counters, padded to 9 dwords
#define FPFH_POINTS 7               // 7 x 33 = 231 of the 256 lanes of a workgroup work
#define FPFH_BLOCK 256
static_assert(NKSR_FPFH_BINS == 33 && SPFH_ROW >= NKSR_FPFH_BINS && SPFH_ROW % 4 == 0 && (SPFH_ROW / 4) % 2 == 1, "33 byte counters, odd dword stride");
static_assert(FPFH_POINTS * NKSR_FPFH_BINS <= FPFH_BLOCK && NKSR_FPFH_MAX_K <= 32, "lanes per point; the mask is one 32-bit word");

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
    const double xy = a[0] * b[0] + a[1] * b[1];
    return xy + a[2] * b[2];
}
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// floor(11 (f + shift) / width) clamped to 0 .. 10 (the clamp in fp64: nothing out of range reaches the conversion)
__device__ __forceinline__ int fpfh_bin(double f, double shift, double width) {
#pragma clang fp contract(off)
    const double s = f + shift;
    const double t = 11.0 * s;
    const double b = floor(t / width);
    return b >= 10.0 ? 10 : (b >= 0.0 ? (int)b : 0);          // (a NaN falls to bin 0)
}

// the three bins of the pair (i, j); false: the cross product vanishes, the pair does not take part
__device__ __forceinline__ bool fpfh_pair(const double xi[3], const double ni[3], const double xj[3], const double nj[3], int bin[3]) {
#pragma clang fp contract(off)
    const double kPi = 3.14159265358979323846;
    double d[3] = {xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2]};
    const double L = sqrt(dot3(d, d));
    const double a1 = dot3(ni, d) / L, a2 = dot3(nj, d) / L;
    const bool swap = fabs(a1) < fabs(a2);
    double u[3], o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = swap ? nj[a] : ni[a];
        o[a] = swap ? ni[a] : nj[a];
        d[a] = swap ? -d[a] : d[a];
    }
    const double f2 = swap ? -a2 : a1;
    double v[3], w[3];
    cross3(d, u, v);
    if (v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0) return false;
    const double lv = sqrt(dot3(v, v));
    v[0] = v[0] / lv;
    v[1] = v[1] / lv;
    v[2] = v[2] / lv;
    cross3(u, v, w);
    const double f1 = dot3(v, o);
    const double f0 = atan2(dot3(w, o), dot3(u, o));
    bin[0] = fpfh_bin(f0, kPi, 2.0 * kPi);
    bin[1] = fpfh_bin(f1, 1.0, 2.0);
    bin[2] = fpfh_bin(f2, 1.0, 2.0);
    return true;
}

__global__ void __launch_bounds__(SPFH_BLOCK) k_spfh(const float* __restrict__ xyz, const float* __restrict__ nrm, int64_t n,
                                                     const int32_t* __restrict__ idx, const float* __restrict__ d2, int k, float r2,
                                                     int32_t* __restrict__ count, int32_t* __restrict__ n_out, uint32_t* __restrict__ mask_out) {
    __shared__ uint8_t s_hist[SPFH_BLOCK][SPFH_ROW];
    const int64_t base = (int64_t)blockIdx.x * SPFH_BLOCK, i = base + threadIdx.x;
    uint32_t* row32 = reinterpret_cast<uint32_t*>(s_hist[threadIdx.x]);
#pragma unroll
    for (int a = 0; a < SPFH_ROW / 4; ++a) row32[a] = 0u;
    if (i < n) {                                        // (a lane touches its own row only: no barrier before the walk)
        uint8_t* row = s_hist[threadIdx.x];
        const double xi[3] = {(double)xyz[i * 3], (double)xyz[i * 3 + 1], (double)xyz[i * 3 + 2]};
        const double ni[3] = {(double)nrm[i * 3], (double)nrm[i * 3 + 1], (double)nrm[i * 3 + 2]};
        uint32_t mask = 0u;
        int cnt = 0;
        for (int m = 0; m < k; ++m) {
            const float dd = d2[i * k + m];
            const int64_t j = idx[i * k + m];
            if (!(dd <= r2) || !(dd > 0.f) || j < 0 || j >= n) continue;         // (an index outside the cloud takes no part)
            const double xj[3] = {(double)xyz[j * 3], (double)xyz[j * 3 + 1], (double)xyz[j * 3 + 2]};
            const double nj[3] = {(double)nrm[j * 3], (double)nrm[j * 3 + 1], (double)nrm[j * 3 + 2]};
            int bin[3];
            if (!fpfh_pair(xi, ni, xj, nj, bin)) continue;
            row[bin[0]] += 1;
            row[11 + bin[1]] += 1;
            row[22 + bin[2]] += 1;
            mask |= 1u << m;
            ++cnt;
        }
        n_out[i] = cnt;
        mask_out[i] = mask;
    }
    __syncthreads();
    const int64_t rest = n - base;
    const int rows = rest < SPFH_BLOCK ? (int)rest : SPFH_BLOCK;
    for (int e = threadIdx.x; e < rows * NKSR_FPFH_BINS; e += SPFH_BLOCK)
        count[base * NKSR_FPFH_BINS + e] = s_hist[e / NKSR_FPFH_BINS][e % NKSR_FPFH_BINS];
}

__global__ void __launch_bounds__(FPFH_BLOCK) k_fpfh(const int32_t* __restrict__ count, const int32_t* __restrict__ n_nb,
                                                     const uint32_t* __restrict__ mask, int64_t n, const int32_t* __restrict__ idx,
                                                     const float* __restrict__ d2, int k, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_f[FPFH_POINTS][NKSR_FPFH_BINS];
    const int p = threadIdx.x / NKSR_FPFH_BINS, b = threadIdx.x % NKSR_FPFH_BINS;
    const int64_t i = (int64_t)blockIdx.x * FPFH_POINTS + p;
    const bool on = p < FPFH_POINTS && i < n;
    double F = 0.0, S = 0.0;
    if (on) {
        const int ni = n_nb[i];
        if (ni > 0) S = (double)count[i * NKSR_FPFH_BINS + b] * (100.0 / (double)ni);
        const uint32_t bits = mask[i];
        for (int m = 0; m < k; ++m) {
            if (!((bits >> m) & 1u)) continue;
            const int64_t j = idx[i * k + m];
            if (j < 0 || j >= n) continue;                  // (nksr_spfh sets no such bit)
            const int nj = n_nb[j];
            const double Sj = nj > 0 ? (double)count[j * NKSR_FPFH_BINS + b] * (100.0 / (double)nj) : 0.0;
            F = F + Sj / (double)d2[i * k + m];
        }
        s_f[p][b] = F;
    }
    __syncthreads();
    if (on) {
        const int g = b / 11;
        double s = 0.0;
        for (int a = 0; a < 11; ++a) s = s + s_f[p][11 * g + a];
        if (s > 0.0) F = F * (100.0 / s);
        out[i * NKSR_FPFH_BINS + b] = (float)(F + S);
    }
}

static int fpfh_args(const char* who, int64_t n, int k) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: n=%lld outside [0, 2^31)", who, (long long)n);
    if (k < 1 || k > NKSR_FPFH_MAX_K) return nksr_set_error(NKSR_ERR_ARG, "%s: k=%d outside [1, %d]", who, k, NKSR_FPFH_MAX_K);
    return NKSR_OK;
}

extern "C" int nksr_spfh(const float* xyz, const float* normal, int64_t n, const int32_t* idx, const float* d2, int k, float radius,
                         int32_t* count_out, int32_t* n_out, uint32_t* mask_out, void* stream) {
    if (int rc = fpfh_args("spfh", n, k)) return rc;
    if (!(radius > 0.f) || !(radius < 3.4e38f)) return nksr_set_error(NKSR_ERR_ARG, "spfh: radius must be positive and finite");
    if (n == 0) return NKSR_OK;
    if (!xyz || !normal || !idx || !d2 || !count_out || !n_out || !mask_out) return nksr_set_error(NKSR_ERR_ARG, "spfh: NULL arrays");
    hipLaunchKernelGGL(k_spfh, dim3(nksr_blocks(n, SPFH_BLOCK)), dim3(SPFH_BLOCK), 0, (hipStream_t)stream, xyz, normal, n, idx, d2, k,
                       radius * radius, count_out, n_out, mask_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_fpfh(const int32_t* count, const int32_t* n_nb, const uint32_t* mask, int64_t n, const int32_t* idx, const float* d2,
                         int k, float* out, void* stream) {
    if (int rc = fpfh_args("fpfh", n, k)) return rc;
    if (n == 0) return NKSR_OK;
    if (!count || !n_nb || !mask || !idx || !d2 || !out) return nksr_set_error(NKSR_ERR_ARG, "fpfh: NULL arrays");
    hipLaunchKernelGGL(k_fpfh, dim3(nksr_blocks(n, FPFH_POINTS)), dim3(FPFH_BLOCK), 0, (hipStream_t)stream, count, n_nb, mask, n, idx, d2, k,
                       out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
