// Voxel reduction of a point cloud: per voxel the mean of xyz and of one [N, C] attribute, the point count and (optionally) the
// point nearest the mean -- nksr_amd/cloud.py voxel_downsample.  The cloud arrives as `order` (point indices sorted by voxel key)
// with the run [start, end) of every voxel in it.
//
// Mapping.  Runs are 1 .. thousands of positions long and the loads are gathers through `order`, so neither a lane per voxel (64
// unequal loops of dependent gathers per wavefront) nor a wavefront per voxel (63 idle lanes on the short runs that make up most of a
// fine grid) fits.  Here a WAVEFRONT owns `group` consecutive voxels, whose runs are one contiguous range of sorted positions, and
// walks that range in tiles of 64: lane = position, so `order` is read coalesced and all 64 gathers of a tile are in flight together.
// Inside a tile every channel is summed by a segmented inclusive scan (segment = voxel, six shuffle steps, a fixed tree) and the
// last lane of each segment adds the segment's tile total to the voxel's fp64 accumulator in LDS; tiles follow each other in
// position order.  The order of every sum is therefore fixed by (start, end, group) alone: no atomics, bitwise repeatable.  A voxel
// with a long run simply spans many tiles of its wavefront (5 000 points: 79 tiles); `group` shrinks with the voxel count so that a
// coarse grid over a large cloud still fills the machine (nksr_voxel_reduce below).
#include "common.h"

#define VR_WAVES 4
#define VR_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct VrTile {
    int seg;            // voxel of this lane's position within the group, -1 past the end of the range
    int idx;            // the point at this position (0 when not live)
    bool live;          // the position belongs to a run and names a point
    bool tail;          // last lane of its segment in this tile
    unsigned same;      // bit b: lane - 2^b is in the same segment
};
// lane `lane` of the tile that starts at sorted position `base`: ss / se = the nv runs of this wavefront (LDS), p1 = end of its range
__device__ __forceinline__ VrTile vr_tile(const int32_t* __restrict__ order, int64_t n, const int* ss, const int* se, int nv, int base, int p1,
                                          int lane) {
    VrTile t;
    const int p = base + lane;
    int seg = 0;                                    // the last run that starts at or before p
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const int s = seg + step;
        if (s < nv && ss[s] <= p) seg = s;
    }
    t.live = p < p1 && p >= ss[seg] && p < se[seg];
    t.seg = p < p1 ? seg : -1;
    t.idx = t.live ? order[p] : 0;
    if (t.idx < 0 || (int64_t)t.idx >= n) { t.live = false; t.idx = 0; }
    t.same = 0u;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const int o = __shfl_up(t.seg, 1 << b);
        if (lane >= (1 << b) && o == t.seg) t.same |= 1u << b;
    }
    const int nxt = __shfl_down(t.seg, 1);
    t.tail = t.seg >= 0 && (lane == 63 || nxt != t.seg);
    return t;
}
__device__ __forceinline__ double vr_scan(double v, unsigned same) {
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const double o = __shfl_up(v, 1 << b);
        if ((same >> b) & 1u) v += o;
    }
    return v;
}

__global__ void __launch_bounds__(64 * VR_WAVES) k_voxel_reduce(const int32_t* __restrict__ order, int64_t n, const int32_t* __restrict__ start,
                                                                const int32_t* __restrict__ end, int64_t nvox, const float* __restrict__ xyz,
                                                                const float* __restrict__ attr, int C, int group, float* __restrict__ mean_xyz,
                                                                float* __restrict__ mean_attr, int32_t* __restrict__ count,
                                                                int32_t* __restrict__ nearest) {
    extern __shared__ double s_vr[];                // per wavefront: acc [64][3 + C], bestd [64], then ss, se, cnt, bestp [64] ints each
    const int NC = 3 + C;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* acc = s_vr + (size_t)wave * (64 * NC + 64 + 128);
    double* bestd = acc + 64 * NC;
    int* ss = reinterpret_cast<int*>(bestd + 64);
    int* se = ss + 64;
    int* cnt = se + 64;
    int* bestp = cnt + 64;
    const int64_t v0 = ((int64_t)blockIdx.x * VR_WAVES + wave) * group;
    if (v0 >= nvox) return;                          // (the whole wavefront: no barrier below spans wavefronts)
    const int nv = (int)(nvox - v0 < group ? nvox - v0 : group);
    if (lane < nv) {
        int s = start[v0 + lane], e = end[v0 + lane];
        s = s < 0 ? 0 : ((int64_t)s > n ? (int)n : s);
        e = e < s ? s : ((int64_t)e > n ? (int)n : e);
        ss[lane] = s; se[lane] = e; cnt[lane] = 0;
        bestd[lane] = 1.0e300; bestp[lane] = -1;
    }
    for (int j = lane; j < nv * NC; j += 64) acc[j] = 0.0;
    VR_SYNC();
    const int p0 = __builtin_amdgcn_readfirstlane(ss[0]), p1 = __builtin_amdgcn_readfirstlane(se[nv - 1]);
    for (int base = p0; base < p1; base += 64) {
        const VrTile t = vr_tile(order, n, ss, se, nv, base, p1, lane);
        const float x = t.live ? xyz[(int64_t)t.idx * 3] : 0.f, y = t.live ? xyz[(int64_t)t.idx * 3 + 1] : 0.f,
                    z = t.live ? xyz[(int64_t)t.idx * 3 + 2] : 0.f;
        int c1 = t.live ? 1 : 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const int o = __shfl_up(c1, 1 << b);
            if ((t.same >> b) & 1u) c1 += o;
        }
        const double sx = vr_scan((double)x, t.same), sy = vr_scan((double)y, t.same), sz = vr_scan((double)z, t.same);
        if (t.tail) {
            cnt[t.seg] += c1;
            acc[t.seg * NC] += sx; acc[t.seg * NC + 1] += sy; acc[t.seg * NC + 2] += sz;
        }
        for (int c0 = 0; c0 < C; c0 += 4) {           // the attribute row four channels at a time: their loads go out together
            float a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = (t.live && c0 + u < C) ? attr[(int64_t)t.idx * C + c0 + u] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= C) break;
                const double s = vr_scan((double)a[u], t.same);
                if (t.tail) acc[t.seg * NC + 3 + c0 + u] += s;
            }
        }
    }
    VR_SYNC();
    for (int j = lane; j < nv * 3; j += 64) {
        const int c = cnt[j / 3];
        mean_xyz[v0 * 3 + j] = c > 0 ? (float)(acc[(j / 3) * NC + j % 3] / (double)c) : 0.f;
    }
    for (int j = lane; j < nv * C; j += 64) {
        const int c = cnt[j / C];
        mean_attr[v0 * C + j] = c > 0 ? (float)(acc[(j / C) * NC + 3 + j % C] / (double)c) : 0.f;
    }
    if (lane < nv) count[v0 + lane] = cnt[lane];
    if (!nearest) return;
    // second walk over the same tiles: squared fp64 distance to the fp64 mean, segmented minimum (the earlier position on a tie: the
    // scan prefers the earlier lane, and a later tile must be strictly nearer)
    VR_SYNC();
    for (int j = lane; j < nv * 3; j += 64) {
        const int c = cnt[j / 3];
        if (c > 0) acc[(j / 3) * NC + j % 3] /= (double)c;
    }
    VR_SYNC();
    for (int base = p0; base < p1; base += 64) {
        const VrTile t = vr_tile(order, n, ss, se, nv, base, p1, lane);
        double d = 1.0e300;
        int bp = base + lane;
        if (t.live) {
            const double ex = (double)xyz[(int64_t)t.idx * 3] - acc[t.seg * NC], ey = (double)xyz[(int64_t)t.idx * 3 + 1] - acc[t.seg * NC + 1],
                         ez = (double)xyz[(int64_t)t.idx * 3 + 2] - acc[t.seg * NC + 2];
            d = ex * ex + ey * ey + ez * ez;
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const double od = __shfl_up(d, 1 << b);
            const int op = __shfl_up(bp, 1 << b);
            if (((t.same >> b) & 1u) && od <= d) { d = od; bp = op; }
        }
        if (t.tail && d < bestd[t.seg]) { bestd[t.seg] = d; bestp[t.seg] = bp; }
    }
    VR_SYNC();
    if (lane < nv) nearest[v0 + lane] = bestp[lane];
}

extern "C" int nksr_voxel_reduce(const int32_t* order, int64_t n, const int32_t* start, const int32_t* end, int64_t n_vox, const float* xyz,
                                 const float* attr, int C, int group, float* mean_xyz_out, float* mean_attr_out, int32_t* count_out,
                                 int32_t* nearest_out, void* stream) {
    if (n < 0 || n_vox < 0 || n > 0x7fffffffll - 64 || n_vox > n)
        return nksr_set_error(NKSR_ERR_ARG, "voxel reduce: 0 <= n_vox <= n < 2^31 (got n=%lld, n_vox=%lld)", (long long)n, (long long)n_vox);
    if (C < 0 || C > NKSR_VOXEL_REDUCE_MAX_C) return nksr_set_error(NKSR_ERR_ARG, "voxel reduce: 0 <= C <= %d channels (got %d)", NKSR_VOXEL_REDUCE_MAX_C, C);
    if (group < 0 || group > 64) return nksr_set_error(NKSR_ERR_ARG, "voxel reduce: group must be 0 (automatic) or 1 .. 64 (got %d)", group);
    if (n_vox == 0) return NKSR_OK;
    if (!order || !start || !end || !xyz || !mean_xyz_out || !count_out) return nksr_set_error(NKSR_ERR_ARG, "voxel reduce: NULL arrays");
    if (C > 0 && (!attr || !mean_attr_out)) return nksr_set_error(NKSR_ERR_ARG, "voxel reduce: C = %d but the attribute arrays are NULL", C);
    if (group == 0)                                  // at least 4096 wavefronts where the voxels allow it, up to 64 voxels per wavefront beyond
        for (group = 64; group > 1 && (n_vox + group - 1) / group < 4096; group >>= 1) {}
    const int64_t waves = (n_vox + group - 1) / group;
    const size_t lds = sizeof(double) * VR_WAVES * (size_t)(64 * (3 + C) + 64 + 128);
    hipLaunchKernelGGL(k_voxel_reduce, dim3(nksr_blocks(waves, VR_WAVES)), dim3(64 * VR_WAVES), lds, (hipStream_t)stream, order, n, start, end,
                       n_vox, xyz, attr, C, group, mean_xyz_out, mean_attr_out, count_out, nearest_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
