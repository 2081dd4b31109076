// Union-find on the device, shared by the mesh components (csrc/meshtopo.hip: hooks over a pair list) and the point-cloud clusters
// (csrc/segment.hip: hooks over the neighbours a grid walk finds): the loads and stores of a parent, the find with path halving, the
// hook of two nodes, and the init / flatten / label kernels round whatever kernel does the hooking.
#pragma once
#include "common.h"

#define UF_BLOCK 256

// DETERMINISM.  A hook only ever points a ROOT at a smaller node of a set it is being joined with (atomicCAS(parent[hi], hi, lo),
// lo < hi), and path halving only replaces a parent by an ancestor.  So at every moment parent[x] <= x, parent[x] lies in the set of
// x, and the smallest node of a set can never receive a parent: whatever order the lanes ran in, once every pair has been hooked each
// tree's root is the MINIMUM NODE INDEX of its component, and the flatten pass (parent[x] = root of x) leaves an array that is a
// function of the graph alone.  Dense ids are the ranks of the roots, so ascending id follows ascending minimum node index.
// A lane may read a stale parent (another CU's L1): every value a parent ever held is an ancestor, so a stale read costs steps, and
// the CAS decides on the word's current value.
__device__ __forceinline__ int32_t uf_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t cur = uf_load(parent + x);
    while (cur != x) {
        const int32_t next = uf_load(parent + cur);
        if (next == cur) return cur;
        uf_store(parent + x, next);                     // path halving: x skips its parent
        x = cur;
        cur = next;
    }
    return cur;
}

// joins the sets of a and b (both nodes of the graph) -> the root the joined set had when the hook went through
__device__ __forceinline__ int32_t uf_hook(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = old;                                        // hi was no root any more: go on from what it points to
        b = lo;
    }
}

static __global__ void __launch_bounds__(UF_BLOCK) k_uf_init(int32_t* __restrict__ parent, int64_t n, const uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * UF_BLOCK + threadIdx.x;
    if (i < n) parent[i] = !valid || valid[i] ? (int32_t)i : -1;
}

static __global__ void __launch_bounds__(UF_BLOCK) k_uf_flatten(int32_t* parent, int64_t n, int32_t* __restrict__ root_flags) {
    const int64_t i = (int64_t)blockIdx.x * UF_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t r = uf_load(parent + i);
    if (r >= 0) {
        while (true) {
            const int32_t p = uf_load(parent + r);
            if (p == r) break;
            r = p;
        }
        if (r != (int32_t)i) uf_store(parent + i, r);   // (a root keeps pointing at itself: other lanes end their walk on it)
    }
    root_flags[i] = r == (int32_t)i ? 1 : 0;
    if (i == 0) root_flags[n] = 0;
}

static __global__ void __launch_bounds__(UF_BLOCK) k_uf_labels(const int32_t* __restrict__ parent, int64_t n, const int32_t* __restrict__ root_rank,
                                                               int32_t* __restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * UF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t r = parent[i];
    label[i] = r >= 0 ? root_rank[r] : -1;
}

#define UF_LAUNCH(kernel, n, st, ...)                                                                                      \
    do {                                                                                                                   \
        hipLaunchKernelGGL(kernel, dim3(nksr_blocks((n), UF_BLOCK)), dim3(UF_BLOCK), 0, (st), __VA_ARGS__);                 \
        NKSR_CHECK_LAUNCH();                                                                                               \
    } while (0)
