// Trilinear splats of per-point values onto the voxels of one level (network.encoder, reference call site models/nksr_net.py:73;
// the U-Net's normal target and the UDF branch, models/nksr_net.py:124-130).
// Gather form (deterministic, no float atomics): voxel j visits the points of its 27 neighbour cells (contiguous ranges of the
// Morton-sorted cloud) and weights them with the hat function  prod_a max(0, 1 - |fl32(x_a * inv_w) - (j_a + 1/2)|).
//   k_splat_trilinear  weighted SUM and weight sum of <= 8 channels, fp64 accumulators      half-wave per voxel, listing pass
//   k_splat_encode32   weighted mean of 32 channels; with normals also their sum as above    half-wave per voxel, listing pass
//   k_splat_mean_c     weighted mean of C != 32 channels                                     thread per (voxel, 8-channel group)
//   k_splat_plane      plane features (centroid offset, mean normal) of the UDF branch       thread per voxel
// The half-wave kernels share SplatHalfWave (the listing pass of common.h), the other two splat_walk_voxel.
#include "launch.h"
// The oracle rounds every fp32 product before it is used (numpy).  Device code contracts a * b + c into one fma by default --
// x * inv_w - centre then keeps the unrounded product, the trilinear weights move by an ulp of p and a splat whose normals nearly
// cancel amplifies that to 1e-4 in the unit target (measured in round 3) -- so contraction is off in this file; explicit fmaf stays.
#pragma clang fp contract(off)

// ---- one 32-lane half-wave per voxel ------------------------------------------------------------------------------------------
// Lane s < 27 = neighbour cell: the 27 chains cell -> point range -> coordinates run side by side (a thread per voxel walks them
// one after the other: latency-bound, 0.68 ms at 7.8e5 voxels) and list the points that weigh at the voxel (common.h:
// splat_for_each_point); then lane = CHANNEL: `consume(k[4], w[4])` gets the listed points four per trip, in list order (cell
// after cell), the same in every lane, so a row of a point is one coalesced read of the half-wave and no sum runs over the lanes.
struct SplatHalfWave {
    int j, s, h;             // voxel, lane of the half-wave, half-wave of the workgroup (256 threads: 8 of them)
    bool live;               // (a dead half-wave walks an empty list next to its partner)
    float cx, cy, cz;        // the voxel's centre, voxel units
    int c;                   // the lane's neighbour cell, -1: none

    __device__ __forceinline__ SplatHalfWave(const int32_t* __restrict__ nbr, const int32_t* __restrict__ ijk, int n)
        : j((blockIdx.x * 256 + threadIdx.x) >> 5), s(threadIdx.x & 31), h(threadIdx.x >> 5), live(j < n) {
        const int jc = live ? j : n - 1;
        cx = (float)ijk[jc * 3] + 0.5f, cy = (float)ijk[jc * 3 + 1] + 0.5f, cz = (float)ijk[jc * 3 + 2] + 0.5f;
        c = (live && s < 27) ? nbr[(int64_t)jc * 27 + s] : -1;
    }
    template <class F>
    __device__ __forceinline__ void for_each_point(const float* __restrict__ xyz, const int32_t* __restrict__ start,
                                                   const int32_t* __restrict__ end, float inv_w, F&& consume) const {
        __shared__ int lk[8][SPLAT_LIST];
        __shared__ float lw[8][SPLAT_LIST];
        splat_for_each_point(xyz, start, end, c, cx, cy, cz, inv_w, s, lk[h], lw[h], consume);
    }
};

// Weighted SUM and weight sum of C <= 8 channels (the splat of the input normals).
// fp64 accumulators: the splat of the input normals is normalised afterwards, and where the normals of a voxel's points nearly
// cancel (both sides of a thin sheet) fp32 sums left 1e-4 of noise in the unit target (round 3: sites with |sum w n| ~ 0.1 sum w
// differed by 7e-5 from the fp64 oracle); the products w * f are exact in fp64, so only the order of the additions is left.
__global__ void __launch_bounds__(256) k_splat_trilinear(const float* __restrict__ xyz, const float* __restrict__ feat, int C,
                                                         const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                                         const int32_t* __restrict__ nbr, const int32_t* __restrict__ ijk, int n,
                                                         float inv_w, float* __restrict__ out, float* __restrict__ wsum_out) {
    const SplatHalfWave v(nbr, ijk, n);
    const int s = v.s, ch = s < C ? s : 0;
    double acc = 0.0, wsum = 0.0;
    v.for_each_point(xyz, start, end, inv_w, [&](const int (&kq)[4], const float (&wq)[4]) {
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = feat[(int64_t)kq[i] * C + ch];
#pragma unroll
        for (int i = 0; i < 4; ++i) { wsum += (double)wq[i]; acc = fma((double)wq[i], (double)f[i], acc); }
    });
    if (v.live && s < C) out[(int64_t)v.j * C + s] = (float)acc;
    if (v.live && s == 0) wsum_out[v.j] = (float)wsum;
}

// The encoder's pass over the points, once for both of its splats: the mean of the 32 feature channels and -- nrm != NULL -- the
// 3-channel weighted SUM of the input normals with its weight sum, as k_splat_trilinear forms them on the same grid.  Both list the
// same points with the same weights in the same order (xyz, inv_w, cell ranges and neighbour rows are the same); only what is read
// per listed point differs, so one listing serves both.  Every lane sums its feature channel in fp32 in list order and stores one
// coalesced 128-byte row per voxel; lanes s < 3 also sum their normal channel in fp64 and round once at the end (the bits of
// k_splat_trilinear: lane 0 carries the weight sum).  Four listed points per trip: 56 VGPRs, 8 waves per SIMD.  More rows in flight
// per wavefront cost more than they gave (HISTORY.md: 8 or 16 points per trip and a prefetch of the next round's candidates need
// 72-128 VGPRs, 7-4 waves per SIMD; 6.9 ms became 7.4-11.0).
__global__ void __launch_bounds__(256) k_splat_encode32(const float* __restrict__ xyz, const float* __restrict__ feat,
                                                        const float* __restrict__ nrm, const int32_t* __restrict__ start,
                                                        const int32_t* __restrict__ end, const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ ijk, int n, float inv_w, float* __restrict__ out,
                                                        float* __restrict__ nsum_out, float* __restrict__ wsum_out) {
    const SplatHalfWave v(nbr, ijk, n);
    const int s = v.s;
    const bool nl = nrm != nullptr && s < 3;                         // this lane sums a normal channel
    float acc = 0.f, wsum = 0.f;
    double nacc = 0.0, nwsum = 0.0;
    v.for_each_point(xyz, start, end, inv_w, [&](const int (&kq)[4], const float (&wq)[4]) {
        float f[4], g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = feat[(int64_t)kq[i] * 32 + s];
        if (nl) {
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = nrm[(int64_t)kq[i] * 3 + s];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { wsum += wq[i]; acc = fmaf(wq[i], f[i], acc); }
        if (nl) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { nwsum += (double)wq[i]; nacc = fma((double)wq[i], (double)g[i], nacc); }
        }
    });
    if (v.live) out[(int64_t)v.j * 32 + s] = acc * (wsum > 0.f ? 1.f / wsum : 0.f);
    if (v.live && nl) nsum_out[(int64_t)v.j * 3 + s] = (float)nacc;
    if (v.live && nl && s == 0) wsum_out[v.j] = (float)nwsum;
}

// ---- one thread per voxel -----------------------------------------------------------------------------------------------------
// The same points in the same order (cell after cell, points in their order), walked by one thread: `f(k, w, rx, ry, rz)` gets
// every point k with three positive weights, its weight and its offset from the voxel's centre in voxel units.
// `f` comes first and by value, and the function is left to the inliner instead of being forced: the closure then reaches the
// kernel as plain values, and an accumulator ARRAY it refers to (k_splat_mean_c) is still turned into registers by the early
// promotion pass, as it was with the walk written out in the kernel.  (A closure passed by reference hides the array from that
// pass: 43 VGPRs instead of 33, a move behind every fma -- profiles/splat_split.md.)
template <class F>
__device__ inline void splat_walk_voxel(F f, const float* __restrict__ xyz, const int32_t* __restrict__ start,
                                        const int32_t* __restrict__ end, const int32_t* __restrict__ nbr,
                                        const int32_t* __restrict__ ijk, int j, float inv_w) {
    const float cx = (float)ijk[j * 3] + 0.5f, cy = (float)ijk[j * 3 + 1] + 0.5f, cz = (float)ijk[j * 3 + 2] + 0.5f;
#pragma unroll 1               // (as the compiler left the loop while it stood in the kernels)
    for (int s = 0; s < 27; ++s) {
        const int c = nbr[(int64_t)j * 27 + s];
        if (c < 0) continue;
        for (int k = start[c]; k < end[c]; ++k) {
            // the hat weight, as the oracle and splat_for_each_point form it: x * inv_w is rounded to fp32 BEFORE the centre is
            // subtracted (contraction is off in this file), and w = (wx * wy) * wz
            const float rx = xyz[(int64_t)k * 3] * inv_w - cx, ry = xyz[(int64_t)k * 3 + 1] * inv_w - cy,
                        rz = xyz[(int64_t)k * 3 + 2] * inv_w - cz;
            const float wx = 1.f - fabsf(rx), wy = 1.f - fabsf(ry), wz = 1.f - fabsf(rz);
            if (wx <= 0.f || wy <= 0.f || wz <= 0.f) continue;
            f(k, wx * wy * wz, rx, ry, rz);
        }
    }
}

// weighted mean of C-channel point features: one thread per (voxel, 8-channel group)
__global__ void k_splat_mean_c(const float* __restrict__ xyz, const float* __restrict__ feat, int C,
                               const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                               const int32_t* __restrict__ nbr, const int32_t* __restrict__ ijk, int n, float inv_w,
                               float* __restrict__ out) {
    const int groups = (C + 7) / 8;
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * groups) return;
    const int j = (int)(t / groups), g = (int)(t % groups);
    const int c0 = g * 8, nc = (C - c0) < 8 ? (C - c0) : 8;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    float wsum = 0.f;
    splat_walk_voxel([&](int k, float w, float, float, float) {
        wsum += w;
        const float* f = feat + (int64_t)k * C + c0;
#pragma unroll
        for (int c2 = 0; c2 < 8; ++c2)
            if (c2 < nc) acc[c2] = fmaf(w, f[c2], acc[c2]);
    }, xyz, start, end, nbr, ijk, j, inv_w);
    const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
    for (int c2 = 0; c2 < nc; ++c2) out[(int64_t)j * C + c0 + c2] = acc[c2] * inv;
}

// UDF mask branch (NeuralField, models/nksr_net.py:124-130): plane features of one level, per voxel j the trilinear-weighted
// centroid offset (voxel units, relative to the voxel centre) and mean normal of the surrounding points.
// out [n, 8] = (occupied, off xyz, unit normal xyz, 0).
__global__ void k_splat_plane(const float* __restrict__ xyz, const float* __restrict__ nrm, const int32_t* __restrict__ start,
                              const int32_t* __restrict__ end, const int32_t* __restrict__ nbr,
                              const int32_t* __restrict__ ijk, int n, float inv_w, float* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    float wsum = 0.f, ox = 0.f, oy = 0.f, oz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    splat_walk_voxel([&](int k, float w, float rx, float ry, float rz) {
        wsum += w;
        ox = fmaf(w, rx, ox); oy = fmaf(w, ry, oy); oz = fmaf(w, rz, oz);
        nx = fmaf(w, nrm[(int64_t)k * 3], nx); ny = fmaf(w, nrm[(int64_t)k * 3 + 1], ny); nz = fmaf(w, nrm[(int64_t)k * 3 + 2], nz);
    }, xyz, start, end, nbr, ijk, j, inv_w);
    float* o = out + (int64_t)j * 8;
    const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
    const float nn = sqrtf(nx * nx + ny * ny + nz * nz);
    const float invn = nn > 1e-8f ? 1.f / nn : 0.f;
    o[0] = wsum > 0.f ? 1.f : 0.f;
    o[1] = ox * inv; o[2] = oy * inv; o[3] = oz * inv;
    o[4] = nx * invn; o[5] = ny * invn; o[6] = nz * invn;
    o[7] = 0.f;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
// (the half-wave kernels carry no point count and read point 0 unconditionally: the callers launch none of them on an empty cloud)
extern "C" int nksr_splat_trilinear(const float* xyz_sorted, const float* feat_sorted, int C, const int32_t* start,
                                    const int32_t* end, const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w,
                                    float* out, float* wsum_out, void* stream) {
    if (C < 1 || C > 8) return nksr_set_error(NKSR_ERR_ARG, "splat supports 1..8 channels");
    if (n <= 0) return NKSR_OK;
    if (!xyz_sorted || !feat_sorted || !start || !end || !nbr || !ijk || !out || !wsum_out) return nksr_set_error(NKSR_ERR_ARG, "splat_trilinear: NULL arrays");
    LAUNCH1D(k_splat_trilinear, (int64_t)n * 32, stream, xyz_sorted, feat_sorted, C, start, end, nbr, ijk, n, inv_w, out, wsum_out);
    return NKSR_OK;
}
extern "C" int nksr_splat_mean(const float* xyz_sorted, const float* feat_sorted, int C, const int32_t* start,
                               const int32_t* end, const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w, float* out,
                               void* stream) {
    if (C < 1 || C > 64) return nksr_set_error(NKSR_ERR_ARG, "splat_mean supports 1..64 channels");
    if (n <= 0) return NKSR_OK;
    if (!xyz_sorted || !feat_sorted || !start || !end || !nbr || !ijk || !out) return nksr_set_error(NKSR_ERR_ARG, "splat_mean: NULL arrays");
    if (C == 32) return nksr_splat_encode(xyz_sorted, feat_sorted, nullptr, start, end, nbr, ijk, n, inv_w, out, nullptr, nullptr, stream);
    LAUNCH1D(k_splat_mean_c, (int64_t)n * ((C + 7) / 8), stream, xyz_sorted, feat_sorted, C, start, end, nbr, ijk, n, inv_w, out);
    return NKSR_OK;
}
extern "C" int nksr_splat_encode(const float* xyz_sorted, const float* feat_sorted, const float* normal_sorted, const int32_t* start,
                                 const int32_t* end, const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w, float* voxel_feat,
                                 float* normal_sum, float* weight_sum, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!xyz_sorted || !feat_sorted || !start || !end || !nbr || !ijk || !voxel_feat) return nksr_set_error(NKSR_ERR_ARG, "splat_encode: NULL arrays");
    if (normal_sorted && (!normal_sum || !weight_sum)) return nksr_set_error(NKSR_ERR_ARG, "splat_encode: NULL normal_sum / weight_sum with normals given");
    LAUNCH1D(k_splat_encode32, (int64_t)n * 32, stream, xyz_sorted, feat_sorted, normal_sorted, start, end, nbr, ijk, n, inv_w, voxel_feat, normal_sum, weight_sum);
    return NKSR_OK;
}
extern "C" int nksr_splat_plane(const float* xyz_sorted, const float* normal_sorted, const int32_t* start, const int32_t* end,
                                const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w, float* out, void* stream) {
    if (n <= 0) return NKSR_OK;
    if (!xyz_sorted || !normal_sorted || !start || !end || !nbr || !ijk || !out) return nksr_set_error(NKSR_ERR_ARG, "splat_plane: NULL arrays");
    LAUNCH1D(k_splat_plane, n, stream, xyz_sorted, normal_sorted, start, end, nbr, ijk, n, inv_w, out);
    return NKSR_OK;
}
