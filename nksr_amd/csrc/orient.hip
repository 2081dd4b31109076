// Normal orientation without sensor positions (nksr_amd/orient.py; definition and round structure in include/nksr_hip.h, DESIGN.md
// section 3.12): the minimum spanning forest of the kNN graph under 1 - |n_i . n_j| by Boruvka rounds that carry a flip parity.
//   k_orient_init      every point its own component
//   k_orient_propose   per component the minimum key among the slots that leave it (64-bit atomicMin, reduced per wavefront first)
//   k_orient_hook      every component links to the one across its best slot, with the parity of the link
//   k_orient_jump      one pointer-doubling step over the links (ping-pong)
//   k_orient_relabel   every point takes its component's new representative and parity
//   k_orient_seeds     per component the seed point (64-bit atomicMax) and the minimum point index (atomicMin)
//   k_orient_apply     global sign per component, the outputs, the inputs of the dense labels
// Every atomic is an integer minimum, maximum or count, so nothing depends on the order the lanes ran in.  One lane per point;
// the kernels are bound by gathers (rep[j], normal[j]) and, without the per-wavefront reduction, by same-address atomics.
#include "common.h"
#include "wave_dev.h"

#define OR_BLOCK 256
#define OR_MAX_GROUPS 4            // distinct representatives a wavefront reduces together; lanes beyond them go one by one
#define OR_NONE 0xFFFFFFFFFFFFFFFFull

// ---- the definition's arithmetic: rounded products and sums, never contracted ------------------------------------------------------
__device__ __forceinline__ float or_dot(float a0, float a1, float a2, float b0, float b1, float b2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}
__device__ __forceinline__ uint32_t or_weight_bits(float dot) {
    const float w = fmaxf(__fsub_rn(1.0f, fabsf(dot)), 0.0f);
    return __float_as_uint(w) & 0x7FFFFFFFu;            // (max(-0, 0) may keep the sign bit: the weight 0 has one bit pattern)
}

__device__ __forceinline__ uint64_t or_load(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (a value of best[] only ever falls inside a round: a stale read is >= the word, so the test never drops a new minimum)
__device__ __forceinline__ void or_min_into(uint64_t* p, uint64_t key) {
    if (key < or_load(p)) atomicMin((unsigned long long*)p, (unsigned long long)key);
}

// ---- reductions over a wavefront --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t or_shfl_xor(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t or_wave_min(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const uint64_t o = or_shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint64_t or_wave_max(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const uint64_t o = or_shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
// The active lanes of a wavefront grouped by label: grouped(l0, mine, leader) runs in EVERY lane once per distinct label (the first
// OR_MAX_GROUPS of them, in the order of their first lane), single() in every active lane that is left.  In Morton order a wavefront
// holds one or two components from the second round on, so a component's word sees one atomic per wavefront instead of one per lane.
template <typename F, typename G>
__device__ __forceinline__ void or_label_groups(int32_t label, bool active, F&& grouped, G&& single) {
    unsigned long long todo = __ballot(active);
    const int lane = threadIdx.x & (NKSR_WAVE - 1);
    for (int g = 0; todo && g < OR_MAX_GROUPS; ++g) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t l0 = __shfl(label, leader);
        const bool mine = active && label == l0;
        grouped(l0, mine, lane == leader);
        todo &= ~__ballot(mine);
    }
    if ((todo >> lane) & 1ull) single();
}

// ---- the round ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OR_BLOCK) k_orient_init(int64_t n, int32_t* __restrict__ rep, uint8_t* __restrict__ par,
                                                          uint8_t* __restrict__ done, uint64_t* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (i >= n) return;
    rep[i] = (int32_t)i;
    par[i] = 0;
    done[i] = 0;
    best[i] = OR_NONE;
}

__global__ void __launch_bounds__(OR_BLOCK) k_orient_propose(const float* __restrict__ normal, const int32_t* __restrict__ idx, int64_t n, int k,
                                                             const int32_t* __restrict__ order, const int32_t* __restrict__ rep,
                                                             uint8_t* __restrict__ done, uint64_t* best, int32_t* counters) {
    const int64_t t = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    int64_t i = t < n ? (order ? (int64_t)order[t] : t) : -1;
    if (i >= n) i = -1;
    const bool active = i >= 0 && !done[i];
    uint64_t own = OR_NONE;
    int32_t ri = 0;
    if (active) {
        ri = rep[i];
        const float a0 = normal[i * 3], a1 = normal[i * 3 + 1], a2 = normal[i * 3 + 2];
        for (int c = 0; c < k; ++c) {
            const uint64_t s = (uint64_t)i * (uint64_t)k + (uint64_t)c;
            const int64_t j = idx[s];
            if (j < 0 || j >= n || j == i) continue;
            const int32_t rj = rep[j];
            if (rj == ri) continue;
            const float dot = or_dot(a0, a1, a2, normal[j * 3], normal[j * 3 + 1], normal[j * 3 + 2]);
            const uint64_t key = ((uint64_t)or_weight_bits(dot) << 32) | s;
            own = key < own ? key : own;
            or_min_into(best + rj, key);                // the other side of the slot
        }
        if (own == OR_NONE) done[i] = 1;                // every neighbour shares the component, and components only grow
    }
    wave_count(active, counters + 1);
    or_label_groups(ri, own != OR_NONE,
                    [&](int32_t l0, bool mine, bool leader) {
                        const uint64_t m = or_wave_min(mine ? own : OR_NONE);
                        if (leader) or_min_into(best + l0, m);
                    },
                    [&]() { or_min_into(best + ri, own); });
}

__global__ void __launch_bounds__(OR_BLOCK) k_orient_hook(const float* __restrict__ normal, const int32_t* __restrict__ idx, int64_t n, int k,
                                                          const int32_t* __restrict__ rep, const uint8_t* __restrict__ par,
                                                          const uint64_t* __restrict__ best, int32_t* __restrict__ link,
                                                          uint8_t* __restrict__ lpar, int32_t* counters) {
    const int64_t i = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    bool hooked = false;
    if (i < n && rep[i] == (int32_t)i) {
        const uint64_t b = best[i];
        int32_t to = (int32_t)i;
        uint8_t p = 0;
        const uint64_t s = b & 0xFFFFFFFFull;
        if (b != OR_NONE && s < (uint64_t)n * (uint64_t)k) {
            const int64_t u = (int64_t)(s / (uint64_t)k), v = idx[s];
            if (v >= 0 && v < n) {
                const int32_t ru = rep[u], rv = rep[v];
                const int32_t other = ru == (int32_t)i ? rv : ru;
                // two components that chose the same slot (keys are distinct: the same key is the same slot) would link to each other
                if (other >= 0 && other < n && other != (int32_t)i && !(best[other] == b && (int32_t)i < other)) {
                    const float dot = or_dot(normal[u * 3], normal[u * 3 + 1], normal[u * 3 + 2], normal[v * 3], normal[v * 3 + 1], normal[v * 3 + 2]);
                    to = other;
                    p = (uint8_t)((par[u] ^ par[v] ^ (dot < 0.0f ? 1 : 0)) & 1);
                    hooked = true;
                }
            }
        }
        link[i] = to;
        lpar[i] = p;
    }
    wave_count(hooked, counters);
}

__global__ void __launch_bounds__(OR_BLOCK) k_orient_jump(const int32_t* __restrict__ rep, int64_t n, const int32_t* __restrict__ link_in,
                                                          const uint8_t* __restrict__ lpar_in, int32_t* __restrict__ link_out,
                                                          uint8_t* __restrict__ lpar_out) {
    const int64_t i = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (i >= n || rep[i] != (int32_t)i) return;
    const int32_t l = link_in[i];
    if (l < 0 || l >= n) return;
    link_out[i] = link_in[l];
    lpar_out[i] = lpar_in[i] ^ lpar_in[l];
}

__global__ void __launch_bounds__(OR_BLOCK) k_orient_relabel(int64_t n, int32_t* __restrict__ rep, uint8_t* __restrict__ par,
                                                             const int32_t* __restrict__ link, const uint8_t* __restrict__ lpar,
                                                             uint64_t* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (i >= n) return;
    best[i] = OR_NONE;
    const int32_t r = rep[i];
    if (r < 0 || r >= n) return;
    rep[i] = link[r];
    par[i] ^= lpar[r];
}

// ---- after the loop ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void or_view(const float* __restrict__ xyz, int64_t i, float vx, float vy, float vz, float t[3]) {
    t[0] = __fsub_rn(vx, xyz[i * 3]);
    t[1] = __fsub_rn(vy, xyz[i * 3 + 1]);
    t[2] = __fsub_rn(vz, xyz[i * 3 + 2]);
}

__global__ void __launch_bounds__(OR_BLOCK) k_orient_seeds(const float* __restrict__ xyz, int64_t n, const int32_t* __restrict__ rep, int mode,
                                                           float vx, float vy, float vz, uint64_t* seed_key, int32_t* min_index) {
    const int64_t i = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    int32_t r = i < n ? rep[i] : -1;
    const bool active = r >= 0 && r < n;
    uint64_t key = 0;
    if (active) {
        uint32_t hi;
        if (mode == NKSR_ORIENT_SEED_VIEWPOINT) {
            float t[3];
            or_view(xyz, i, vx, vy, vz, t);
            hi = 0xFFFFFFFFu - __float_as_uint(or_dot(t[0], t[1], t[2], t[0], t[1], t[2]));       // nearest first
        } else {
            hi = ordered_bits(xyz[i * 3 + 2]);
        }
        key = ((uint64_t)hi << 32) | (uint64_t)(~(uint32_t)i);
    }
    or_label_groups(r, active,
                    [&](int32_t l0, bool mine, bool leader) {
                        const uint64_t mx = or_wave_max(mine ? key : 0ull);
                        const uint64_t mn = or_wave_min(mine ? (uint64_t)i : OR_NONE);
                        if (leader) {
                            if (mx > or_load(seed_key + l0)) atomicMax((unsigned long long*)(seed_key + l0), (unsigned long long)mx);
                            atomicMin(min_index + l0, (int32_t)mn);
                        }
                    },
                    [&]() {
                        atomicMax((unsigned long long*)(seed_key + r), (unsigned long long)key);
                        atomicMin(min_index + r, (int32_t)i);
                    });
}

__global__ void __launch_bounds__(OR_BLOCK) k_orient_apply(const float* __restrict__ xyz, const float* __restrict__ normal, int64_t n,
                                                           const int32_t* __restrict__ rep, const uint8_t* __restrict__ par,
                                                           const uint64_t* __restrict__ seed_key, const int32_t* __restrict__ min_index, int mode,
                                                           float vx, float vy, float vz, uint8_t* __restrict__ flipped, float* __restrict__ normal_out,
                                                           int32_t* __restrict__ parent, int32_t* __restrict__ root_flags) {
    const int64_t i = (int64_t)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (i == 0) root_flags[n] = 0;
    int32_t r = rep[i];
    if (r < 0 || r >= n) r = (int32_t)i;
    int64_t s = (int64_t)(~(uint32_t)(seed_key[r] & 0xFFFFFFFFull));
    if (s >= n) s = i;
    bool seed_flip;
    if (mode == NKSR_ORIENT_SEED_VIEWPOINT) {
        float t[3];
        or_view(xyz, s, vx, vy, vz, t);
        seed_flip = or_dot(normal[s * 3], normal[s * 3 + 1], normal[s * 3 + 2], t[0], t[1], t[2]) < 0.0f;
    } else {
        seed_flip = normal[s * 3 + 2] < 0.0f;
    }
    const bool f = ((par[i] ^ par[s]) & 1) != (seed_flip ? 1 : 0);
    flipped[i] = f ? 1 : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) normal_out[i * 3 + a] = f ? -normal[i * 3 + a] : normal[i * 3 + a];
    const int32_t m = min_index[r];
    parent[i] = m;
    root_flags[i] = m == (int32_t)i ? 1 : 0;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
#define OR_LAUNCH(kernel, n, st, ...)                                                                                    \
    do {                                                                                                                 \
        hipLaunchKernelGGL(kernel, dim3(nksr_blocks((n), OR_BLOCK)), dim3(OR_BLOCK), 0, (st), __VA_ARGS__);               \
        NKSR_CHECK_LAUNCH();                                                                                             \
    } while (0)

static int or_check_n(const char* what, int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: n=%lld outside [0, 2^31)", what, (long long)n);
    return NKSR_OK;
}
static int or_check_graph(const char* what, int64_t n, int k) {
    int rc = or_check_n(what, n);
    if (rc) return rc;
    if (k < 1 || k > NKSR_ORIENT_MAX_K) return nksr_set_error(NKSR_ERR_ARG, "%s: 1 <= k <= %d (got %d)", what, NKSR_ORIENT_MAX_K, k);
    if (n * (int64_t)k >= (1ll << 32)) return nksr_set_error(NKSR_ERR_ARG, "%s: n k = %lld slots do not fit 32 bits", what, (long long)(n * k));
    return NKSR_OK;
}
static int or_check_mode(const char* what, int mode, float vx, float vy, float vz) {
    if (mode != NKSR_ORIENT_SEED_Z && mode != NKSR_ORIENT_SEED_VIEWPOINT) return nksr_set_error(NKSR_ERR_ARG, "%s: unknown seed mode %d", what, mode);
    if (mode == NKSR_ORIENT_SEED_VIEWPOINT && !(fabsf(vx) < INFINITY && fabsf(vy) < INFINITY && fabsf(vz) < INFINITY))
        return nksr_set_error(NKSR_ERR_ARG, "%s: the viewpoint must be finite", what);
    return NKSR_OK;
}

extern "C" int nksr_orient_init(int64_t n, int32_t* rep, uint8_t* par, uint8_t* done, uint64_t* best, void* stream) {
    int rc = or_check_n("orient init", n);
    if (rc) return rc;
    if (n == 0) return NKSR_OK;
    if (!rep || !par || !done || !best) return nksr_set_error(NKSR_ERR_ARG, "orient init: NULL arrays");
    OR_LAUNCH(k_orient_init, n, (hipStream_t)stream, n, rep, par, done, best);
    return NKSR_OK;
}

extern "C" int nksr_orient_propose(const float* normal, const int32_t* idx, int64_t n, int k, const int32_t* order, const int32_t* rep, uint8_t* done,
                                   uint64_t* best, int32_t* counters, void* stream) {
    int rc = or_check_graph("orient propose", n, k);
    if (rc) return rc;
    if (n == 0) return NKSR_OK;
    if (!normal || !idx || !rep || !done || !best || !counters) return nksr_set_error(NKSR_ERR_ARG, "orient propose: NULL arrays");
    OR_LAUNCH(k_orient_propose, n, (hipStream_t)stream, normal, idx, n, k, order, rep, done, best, counters);
    return NKSR_OK;
}

extern "C" int nksr_orient_hook(const float* normal, const int32_t* idx, int64_t n, int k, const int32_t* rep, const uint8_t* par, const uint64_t* best,
                                int32_t* link_out, uint8_t* lpar_out, int32_t* counters, void* stream) {
    int rc = or_check_graph("orient hook", n, k);
    if (rc) return rc;
    if (n == 0) return NKSR_OK;
    if (!normal || !idx || !rep || !par || !best || !link_out || !lpar_out || !counters) return nksr_set_error(NKSR_ERR_ARG, "orient hook: NULL arrays");
    OR_LAUNCH(k_orient_hook, n, (hipStream_t)stream, normal, idx, n, k, rep, par, best, link_out, lpar_out, counters);
    return NKSR_OK;
}

extern "C" int nksr_orient_jump(const int32_t* rep, int64_t n, const int32_t* link_in, const uint8_t* lpar_in, int32_t* link_out, uint8_t* lpar_out,
                                void* stream) {
    int rc = or_check_n("orient jump", n);
    if (rc) return rc;
    if (n == 0) return NKSR_OK;
    if (!rep || !link_in || !lpar_in || !link_out || !lpar_out) return nksr_set_error(NKSR_ERR_ARG, "orient jump: NULL arrays");
    if (link_in == link_out || lpar_in == lpar_out) return nksr_set_error(NKSR_ERR_ARG, "orient jump: the step reads and writes different buffers");
    OR_LAUNCH(k_orient_jump, n, (hipStream_t)stream, rep, n, link_in, lpar_in, link_out, lpar_out);
    return NKSR_OK;
}

extern "C" int nksr_orient_relabel(int64_t n, int32_t* rep, uint8_t* par, const int32_t* link, const uint8_t* lpar, uint64_t* best, void* stream) {
    int rc = or_check_n("orient relabel", n);
    if (rc) return rc;
    if (n == 0) return NKSR_OK;
    if (!rep || !par || !link || !lpar || !best) return nksr_set_error(NKSR_ERR_ARG, "orient relabel: NULL arrays");
    OR_LAUNCH(k_orient_relabel, n, (hipStream_t)stream, n, rep, par, link, lpar, best);
    return NKSR_OK;
}

extern "C" int nksr_orient_seeds(const float* xyz, int64_t n, const int32_t* rep, int mode, float vx, float vy, float vz, uint64_t* seed_key,
                                 int32_t* min_index, void* stream) {
    int rc = or_check_n("orient seeds", n);
    if (rc) return rc;
    if ((rc = or_check_mode("orient seeds", mode, vx, vy, vz))) return rc;
    if (n == 0) return NKSR_OK;
    if (!xyz || !rep || !seed_key || !min_index) return nksr_set_error(NKSR_ERR_ARG, "orient seeds: NULL arrays");
    OR_LAUNCH(k_orient_seeds, n, (hipStream_t)stream, xyz, n, rep, mode, vx, vy, vz, seed_key, min_index);
    return NKSR_OK;
}

extern "C" int nksr_orient_apply(const float* xyz, const float* normal, int64_t n, const int32_t* rep, const uint8_t* par, const uint64_t* seed_key,
                                 const int32_t* min_index, int mode, float vx, float vy, float vz, uint8_t* flipped_out, float* normal_out,
                                 int32_t* parent_out, int32_t* root_flags_out, void* stream) {
    int rc = or_check_n("orient apply", n);
    if (rc) return rc;
    if ((rc = or_check_mode("orient apply", mode, vx, vy, vz))) return rc;
    if (!root_flags_out) return nksr_set_error(NKSR_ERR_ARG, "orient apply: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { NKSR_CHECK_HIP(hipMemsetAsync(root_flags_out, 0, sizeof(int32_t), st)); return NKSR_OK; }
    if (!xyz || !normal || !rep || !par || !seed_key || !min_index || !flipped_out || !normal_out || !parent_out)
        return nksr_set_error(NKSR_ERR_ARG, "orient apply: NULL arrays");
    OR_LAUNCH(k_orient_apply, n, st, xyz, normal, n, rep, par, seed_key, min_index, mode, vx, vy, vz, flipped_out, normal_out, parent_out, root_flags_out);
    return NKSR_OK;
}
