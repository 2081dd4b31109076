// Triangle-mesh topology (nksr_amd/mesh_topology.py: MeshTopology; layouts in include/nksr_hip.h):
//   k_topo_keys         three (edge key, half-edge id) pairs per face; validity of faces, referenced vertices
//   (the runs of the sorted keys: nksr_run_counts_u64 / nksr_run_table_u64 of csrc/prims.hip, keys from the sentinel on in no run)
//   k_topo_edge_classes edge_v, incident faces, class, the face across every manifold half-edge, totals
//   k_uf_*              union-find over a node and pair list: hook (atomicCAS, larger root under smaller), flatten, dense labels (uf_dev.h)
//   k_topo_*            labels of the other kind of node, per-component counts and boxes, compaction
// Every kernel is one lane per item, latency- and atomic-bound; no sum here is a floating-point one.
#include "common.h"
#include "mesh_dev.h"
#include "uf_dev.h"
#include "wave_dev.h"
static_assert(UF_BLOCK == MESH_BLOCK, "the union-find kernels are launched with MESH_LAUNCH here");

// the key no edge has and that sorts behind every edge of a mesh of nv vertices, inside the 32 + bit_length(nv) sorted bits
__device__ __forceinline__ uint64_t tp_sentinel(int64_t nv) { return ((uint64_t)nv << 32) | (uint64_t)nv; }

// The lanes of a wavefront that carry the same label act together: f(label, lanes of the group, am I its first lane, am I in it) once per
// distinct label, so a component's counters see one atomic per wavefront and label instead of one per lane (a mesh of a few
// components would otherwise queue every face on the same few words).  Every lane of the wavefront must call it.
template <typename F>
__device__ __forceinline__ void tp_label_groups(int32_t label, bool active, F&& f) {
    unsigned long long todo = __ballot(active);
    const int lane = threadIdx.x & (NKSR_WAVE - 1);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t l0 = __shfl(label, leader);
        const bool mine = active && label == l0;
        const unsigned long long group = __ballot(mine);
        f(l0, group, lane == leader, mine);
        todo &= ~group;
    }
}
__device__ __forceinline__ void tp_add_by_label(int32_t label, bool active, int64_t* counts, int column) {
    tp_label_groups(label, active, [&](int32_t l0, unsigned long long group, bool first, bool) {
        if (first) atomicAdd((unsigned long long*)(counts + (int64_t)l0 * 4 + column), (unsigned long long)__popcll(group));
    });
}

// ---- 1. half-edge keys -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_keys(const void* faces, int is64, int64_t nf, int64_t nv, uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ ids, uint8_t* __restrict__ face_valid,
                                                          uint8_t* __restrict__ vertex_ref) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= nf) return;
    int64_t c[3];
    const bool ok = mesh_valid_face(faces, is64, j, nv, c);
    face_valid[j] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t a = c[k], b = c[k == 2 ? 0 : k + 1];
        keys[j * 3 + k] = ok ? ((uint64_t)(a < b ? a : b) << 32) | (uint64_t)(a < b ? b : a) : tp_sentinel(nv);
        ids[j * 3 + k] = (uint32_t)(j * 3 + k);
        if (ok) vertex_ref[a] = 1;                      // (every writer stores the same byte)
    }
}

// ---- 3. edge classes (edge e = run e of the sorted keys: edge_keys = the runs' keys, edge_start their starts) --------------------
__device__ __forceinline__ bool tp_forward(const void* faces, int is64, uint32_t h) {      // does half-edge h run min -> max?
    const int64_t f = h / 3u;
    const int k = (int)(h % 3u);
    return mesh_face_index(faces, is64, f * 3 + k) < mesh_face_index(faces, is64, f * 3 + (k == 2 ? 0 : k + 1));
}

// edge_v[e] = (min, max) of the edge's key; totals: [0] E, [1] boundary, [2] non-manifold, [3] misoriented edges (integer atomics)
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_edge_classes(const void* faces, int is64, const uint32_t* __restrict__ ids,
                                                                  const uint64_t* __restrict__ edge_keys, const uint32_t* __restrict__ edge_start,
                                                                  int64_t ne, int32_t* __restrict__ edge_v, int32_t* __restrict__ edge_count,
                                                                  uint8_t* __restrict__ edge_class, int32_t* __restrict__ face_adj,
                                                                  int64_t* __restrict__ totals) {
    const int64_t e = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    int cls = 0;
    if (e < ne) {
        const uint64_t k = edge_keys[e];
        edge_v[e * 2] = (int32_t)(k >> 32);
        edge_v[e * 2 + 1] = (int32_t)(k & 0xFFFFFFFFull);
        const uint32_t s = edge_start[e];
        const uint32_t cnt = edge_start[e + 1] - s;
        cls = cnt == 1 ? NKSR_TOPO_BOUNDARY : (cnt > 2 ? NKSR_TOPO_NONMANIFOLD : NKSR_TOPO_INTERIOR);
        if (cnt == 2) {
            const uint32_t h0 = ids[s], h1 = ids[(int64_t)s + 1];
            if (tp_forward(faces, is64, h0) == tp_forward(faces, is64, h1)) cls = NKSR_TOPO_MISORIENTED;
            face_adj[h0] = (int32_t)(h1 / 3u);
            face_adj[h1] = (int32_t)(h0 / 3u);
        }
        edge_count[e] = (int32_t)cnt;
        edge_class[e] = (uint8_t)cls;
    }
    wave_count(cls == NKSR_TOPO_BOUNDARY, totals + 1);
    wave_count(cls == NKSR_TOPO_NONMANIFOLD, totals + 2);
    wave_count(cls == NKSR_TOPO_MISORIENTED, totals + 3);
}

__global__ void __launch_bounds__(MESH_BLOCK) k_topo_count_bytes(const uint8_t* __restrict__ flags, int64_t n, int64_t* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    wave_count(i < n && flags[i] != 0, total);
}

// totals[4] = invalid faces (the sentinel half-edges / 3), totals[0] = E
__global__ void k_topo_finish_totals(const uint32_t* __restrict__ edge_start, int64_t ne, int64_t n_half, int64_t* __restrict__ totals) {
    totals[0] = ne;
    totals[4] = (n_half - (ne > 0 || n_half > 0 ? (int64_t)edge_start[ne] : 0)) / 3;
}

// ---- 4. union-find (the device functions, the determinism argument and k_uf_init / k_uf_flatten / k_uf_labels: uf_dev.h) -------------
__global__ void __launch_bounds__(MESH_BLOCK) k_uf_hook(int32_t* parent, int64_t n, const int32_t* __restrict__ pairs, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= m) return;
    const int32_t a = pairs[i * 2], b = pairs[i * 2 + 1];
    if (a < 0 || b < 0 || a >= n || b >= n || a == b) return;
    if (parent[a] < 0 || parent[b] < 0) return;         // (a node outside the graph: -1 is written before the hooks and never changes)
    uf_hook(parent, a, b);
}

// the faces round an edge, linked in a chain: pair i = (face of sorted half-edge i, face of half-edge i + 1) inside a run, else (-1, -1)
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_face_pairs(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ids, int64_t n,
                                                                int64_t nv, int32_t* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    const bool link = i + 1 < n && k != tp_sentinel(nv) && keys[i + 1] == k;
    pairs[i * 2] = link ? (int32_t)(ids[i] / 3u) : -1;
    pairs[i * 2 + 1] = link ? (int32_t)(ids[i + 1] / 3u) : -1;
}

// ---- labels of the other kind of node --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_vertex_min_label(const void* faces, int is64, int64_t nf, int64_t nv,
                                                                      const int32_t* __restrict__ face_label, int32_t* vertex_label) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= nf) return;
    const int32_t l = face_label[j];
    if (l < 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicMin(vertex_label + mesh_face_index(faces, is64, j * 3 + k), l);
}
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_fix_unlabelled(int32_t* __restrict__ label, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n && label[i] == 0x7F7F7F7F) label[i] = -1;
}
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_face_from_vertex(const void* faces, int is64, int64_t nf, const uint8_t* __restrict__ face_valid,
                                                                      const int32_t* __restrict__ vertex_label, int32_t* __restrict__ face_label) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= nf) return;
    face_label[j] = face_valid[j] ? vertex_label[mesh_face_index(faces, is64, j * 3)] : -1;
}

// ---- 5. per-component statistics -------------------------------------------------------------------------------------------------
// counts [n_comp, 4] int64: faces, vertices, edges, boundary edges.  A vertex is counted here in the component of its label; the
// corners whose face lies in another component are the "shared corners" below.
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_component_counts(const int32_t* __restrict__ face_label, int64_t nf,
                                                                      const int32_t* __restrict__ vertex_label, int64_t nv,
                                                                      const uint32_t* __restrict__ ids, const uint32_t* __restrict__ edge_start,
                                                                      const uint8_t* __restrict__ edge_class, int64_t ne, int64_t n_comp,
                                                                      int64_t* counts) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int32_t lf = i < nf ? face_label[i] : -1;
    tp_add_by_label(lf, lf >= 0 && lf < n_comp, counts, 0);
    const int32_t lv = i < nv ? vertex_label[i] : -1;
    tp_add_by_label(lv, lv >= 0 && lv < n_comp, counts, 1);
    const int32_t le = i < ne ? face_label[ids[edge_start[i]] / 3u] : -1;      // every face round an edge lies in one component
    const bool on = le >= 0 && le < n_comp;
    tp_add_by_label(le, on, counts, 2);
    tp_add_by_label(le, on && edge_class[i] == NKSR_TOPO_BOUNDARY, counts, 3);
}

// corner (face j, k) whose vertex carries another component's label (components that only touch at a vertex): key = (label << 32) | v
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_shared_corners(const void* faces, int is64, int64_t nf, const int32_t* __restrict__ face_label,
                                                                    const int32_t* __restrict__ vertex_label, uint64_t* __restrict__ keys,
                                                                    int64_t capacity, int64_t* count) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= nf) return;
    const int32_t l = face_label[j];
    if (l < 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t v = mesh_face_index(faces, is64, j * 3 + k);
        if (vertex_label[v] == l) continue;
        const int64_t pos = (int64_t)atomicAdd((unsigned long long*)count, 1ull);
        if (keys && pos < capacity) keys[pos] = ((uint64_t)(uint32_t)l << 32) | (uint64_t)v;     // (any order: the list is sorted next)
    }
}
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_count_shared(const uint64_t* __restrict__ keys, int64_t m, int64_t n_comp, int64_t* counts) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = keys[i];
    const int64_t l = (int64_t)(k >> 32);
    if ((i == 0 || keys[i - 1] != k) && l < n_comp) atomicAdd((unsigned long long*)(counts + l * 4 + 1), 1ull);
}

// boxes as order-preserving integers (ordered_bits / ordered_float: wave_dev.h)
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_box_init(uint32_t* __restrict__ box, int64_t n_comp) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n_comp * 6) box[i] = i % 6 < 3 ? 0xFFFFFFFFu : 0u;
}
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_box_faces(const float* __restrict__ v, const void* faces, int is64, int64_t nf,
                                                               const int32_t* __restrict__ face_label, int64_t n_comp, uint32_t* box) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int32_t l = j < nf ? face_label[j] : -1;
    const bool on = l >= 0 && l < n_comp;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (on) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t vi = mesh_face_index(faces, is64, j * 3 + k);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint32_t x = ordered_bits(v[vi * 3 + a]);
                lo[a] = x < lo[a] ? x : lo[a];
                hi[a] = x > hi[a] ? x : hi[a];
            }
        }
    }
    tp_label_groups(l, on, [&](int32_t l0, unsigned long long, bool first, bool mine) {
        uint32_t glo[3], ghi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { glo[a] = mine ? lo[a] : 0xFFFFFFFFu; ghi[a] = mine ? hi[a] : 0u; }
#pragma unroll
        for (int off = NKSR_WAVE / 2; off > 0; off >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint32_t p = __shfl_xor(glo[a], off), q = __shfl_xor(ghi[a], off);
                glo[a] = p < glo[a] ? p : glo[a];
                ghi[a] = q > ghi[a] ? q : ghi[a];
            }
        if (first)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(box + (int64_t)l0 * 6 + a, glo[a]);
                atomicMax(box + (int64_t)l0 * 6 + 3 + a, ghi[a]);
            }
    });
}
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_box_decode(uint32_t* __restrict__ box, int64_t n_comp) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n_comp * 6) box[i] = __float_as_uint(ordered_float(box[i]));
}

// ---- 6. compaction ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_mark(const void* faces, int is64, int64_t nf, int64_t nv, const uint8_t* __restrict__ keep,
                                                          int32_t* __restrict__ face_flags, int32_t* __restrict__ vertex_flags) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j == 0) { face_flags[nf] = 0; }
    if (j >= nf) return;
    int64_t c[3];
    const bool on = keep[j] != 0 && mesh_valid_face(faces, is64, j, nv, c);
    face_flags[j] = on ? 1 : 0;
    if (on) { vertex_flags[c[0]] = 1; vertex_flags[c[1]] = 1; vertex_flags[c[2]] = 1; }
}
__global__ void __launch_bounds__(MESH_BLOCK) k_topo_renumber(const void* faces, int is64, int64_t nf, int64_t nv, const int32_t* __restrict__ face_flags,
                                                              const int32_t* __restrict__ face_offsets, const int32_t* __restrict__ vertex_flags,
                                                              const int32_t* __restrict__ vertex_offsets, void* faces_out,
                                                              int64_t* __restrict__ vertex_map) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < nv) vertex_map[i] = vertex_flags[i] ? (int64_t)vertex_offsets[i] : -1;
    if (i < nf && face_flags[i]) {
        const int64_t o = face_offsets[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int32_t w = vertex_offsets[mesh_face_index(faces, is64, i * 3 + k)];
            if (is64) ((int64_t*)faces_out)[o * 3 + k] = w;
            else ((int32_t*)faces_out)[o * 3 + k] = w;
        }
    }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int nksr_topo_halfedge_keys(const void* faces, int faces_int64, int64_t nf, int64_t nv, uint64_t* keys_out, uint32_t* ids_out,
                                       uint8_t* face_valid_out, uint8_t* vertex_ref_out, void* stream) {
    int rc = mesh_check_sizes("topo keys", nv, nf);
    if (rc) return rc;
    if ((nf > 0 && (!faces || !keys_out || !ids_out || !face_valid_out)) || (nv > 0 && !vertex_ref_out))
        return nksr_set_error(NKSR_ERR_ARG, "topo keys: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (nv > 0) NKSR_CHECK_HIP(hipMemsetAsync(vertex_ref_out, 0, (size_t)nv, st));
    if (nf > 0) MESH_LAUNCH(k_topo_keys, nf, st, faces, faces_int64, nf, nv, keys_out, ids_out, face_valid_out, vertex_ref_out);
    return NKSR_OK;
}

static int tp_check_half(const char* who, int64_t n_half, int64_t nv) {
    if (n_half < 0 || n_half % 3 != 0) return nksr_set_error(NKSR_ERR_ARG, "%s: n_half=%lld is not three times a face count", who, (long long)n_half);
    return mesh_check_sizes(who, nv, n_half / 3);
}

extern "C" int nksr_topo_edge_classes(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint32_t* ids_sorted,
                                      const uint64_t* edge_keys, const uint32_t* edge_start, int64_t n_edges, const uint8_t* vertex_ref,
                                      int32_t* edge_v_out, int32_t* edge_count_out, uint8_t* edge_class_out, int32_t* face_adj_out,
                                      int64_t* totals_out, void* stream) {
    int rc = mesh_check_sizes("topo edge classes", nv, nf);
    if (rc) return rc;
    if (n_edges < 0 || n_edges > 3 * nf) return nksr_set_error(NKSR_ERR_ARG, "topo edge classes: n_edges=%lld of %lld faces", (long long)n_edges, (long long)nf);
    if (!totals_out || !edge_start || (nf > 0 && (!faces || !ids_sorted || !face_adj_out)) || (nv > 0 && !vertex_ref) ||
        (n_edges > 0 && (!edge_keys || !edge_v_out || !edge_count_out || !edge_class_out)))
        return nksr_set_error(NKSR_ERR_ARG, "topo edge classes: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(totals_out, 0, sizeof(int64_t) * NKSR_TOPO_TOTALS, st));
    if (nf > 0) NKSR_CHECK_HIP(hipMemsetAsync(face_adj_out, 0xFF, sizeof(int32_t) * 3 * (size_t)nf, st));
    if (n_edges > 0)
        MESH_LAUNCH(k_topo_edge_classes, n_edges, st, faces, faces_int64, ids_sorted, edge_keys, edge_start, n_edges, edge_v_out, edge_count_out,
                    edge_class_out, face_adj_out, totals_out);
    if (nv > 0) MESH_LAUNCH(k_topo_count_bytes, nv, st, vertex_ref, nv, totals_out + 5);
    hipLaunchKernelGGL(k_topo_finish_totals, dim3(1), dim3(1), 0, st, edge_start, n_edges, 3 * nf, totals_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_topo_face_pairs(const uint64_t* keys_sorted, const uint32_t* ids_sorted, int64_t n_half, int64_t nv, int32_t* pairs_out,
                                    void* stream) {
    int rc = tp_check_half("topo face pairs", n_half, nv);
    if (rc) return rc;
    if (n_half == 0) return NKSR_OK;
    if (!keys_sorted || !ids_sorted || !pairs_out) return nksr_set_error(NKSR_ERR_ARG, "topo face pairs: NULL arrays");
    MESH_LAUNCH(k_topo_face_pairs, n_half, (hipStream_t)stream, keys_sorted, ids_sorted, n_half, nv, pairs_out);
    return NKSR_OK;
}

extern "C" int nksr_uf_components(int32_t* parent, int64_t n, const uint8_t* valid, const int32_t* pairs, int64_t n_pairs, int32_t* root_flags_out,
                                  void* stream) {
    if (n < 0 || n_pairs < 0) return nksr_set_error(NKSR_ERR_ARG, "union-find: negative size (n=%lld, pairs=%lld)", (long long)n, (long long)n_pairs);
    if (n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "union-find: %lld nodes do not fit int32 parents", (long long)n);
    if (!root_flags_out || (n > 0 && !parent) || (n_pairs > 0 && !pairs)) return nksr_set_error(NKSR_ERR_ARG, "union-find: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { NKSR_CHECK_HIP(hipMemsetAsync(root_flags_out, 0, sizeof(int32_t), st)); return NKSR_OK; }
    MESH_LAUNCH(k_uf_init, n, st, parent, n, valid);
    if (n_pairs > 0) MESH_LAUNCH(k_uf_hook, n_pairs, st, parent, n, pairs, n_pairs);
    MESH_LAUNCH(k_uf_flatten, n, st, parent, n, root_flags_out);
    return NKSR_OK;
}

extern "C" int nksr_uf_labels(const int32_t* parent, int64_t n, const int32_t* root_rank, int32_t* label_out, void* stream) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "union-find labels: n=%lld outside [0, 2^31)", (long long)n);
    if (n == 0) return NKSR_OK;
    if (!parent || !root_rank || !label_out) return nksr_set_error(NKSR_ERR_ARG, "union-find labels: NULL arrays");
    MESH_LAUNCH(k_uf_labels, n, (hipStream_t)stream, parent, n, root_rank, label_out);
    return NKSR_OK;
}

extern "C" int nksr_topo_cross_labels(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint8_t* face_valid, int from_vertices,
                                      int32_t* face_label, int32_t* vertex_label, void* stream) {
    int rc = mesh_check_sizes("topo cross labels", nv, nf);
    if (rc) return rc;
    if ((nf > 0 && (!faces || !face_valid || !face_label)) || (nv > 0 && !vertex_label)) return nksr_set_error(NKSR_ERR_ARG, "topo cross labels: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (from_vertices) {
        if (nf > 0) MESH_LAUNCH(k_topo_face_from_vertex, nf, st, faces, faces_int64, nf, face_valid, vertex_label, face_label);
        return NKSR_OK;
    }
    if (nv == 0) return NKSR_OK;
    NKSR_CHECK_HIP(hipMemsetAsync(vertex_label, 0x7F, sizeof(int32_t) * (size_t)nv, st));
    if (nf > 0) MESH_LAUNCH(k_topo_vertex_min_label, nf, st, faces, faces_int64, nf, nv, face_label, vertex_label);
    MESH_LAUNCH(k_topo_fix_unlabelled, nv, st, vertex_label, nv);
    return NKSR_OK;
}

extern "C" int nksr_topo_component_counts(const int32_t* face_label, int64_t nf, const int32_t* vertex_label, int64_t nv, const uint32_t* ids_sorted,
                                          const uint32_t* edge_start, const uint8_t* edge_class, int64_t n_edges, int64_t n_comp,
                                          int64_t* counts_out, void* stream) {
    int rc = mesh_check_sizes("topo component counts", nv, nf);
    if (rc) return rc;
    if (n_edges < 0 || n_comp < 0) return nksr_set_error(NKSR_ERR_ARG, "topo component counts: negative size");
    if (n_comp == 0) return NKSR_OK;
    if (!counts_out || (nf > 0 && !face_label) || (nv > 0 && !vertex_label) || (n_edges > 0 && (!ids_sorted || !edge_start || !edge_class)))
        return nksr_set_error(NKSR_ERR_ARG, "topo component counts: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(counts_out, 0, sizeof(int64_t) * 4 * (size_t)n_comp, st));
    const int64_t n = nf > nv ? (nf > n_edges ? nf : n_edges) : (nv > n_edges ? nv : n_edges);
    if (n > 0)
        MESH_LAUNCH(k_topo_component_counts, n, st, face_label, nf, vertex_label, nv, ids_sorted, edge_start, edge_class, n_edges, n_comp, counts_out);
    return NKSR_OK;
}

extern "C" int nksr_topo_shared_corners(const void* faces, int faces_int64, int64_t nf, int64_t nv, const int32_t* face_label,
                                        const int32_t* vertex_label, uint64_t* keys_out, int64_t capacity, int64_t* count_out, void* stream) {
    int rc = mesh_check_sizes("topo shared corners", nv, nf);
    if (rc) return rc;
    if (capacity < 0) return nksr_set_error(NKSR_ERR_ARG, "topo shared corners: negative capacity");
    if (!count_out || (nf > 0 && (!faces || !face_label || !vertex_label)) || (capacity > 0 && !keys_out))
        return nksr_set_error(NKSR_ERR_ARG, "topo shared corners: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), st));
    if (nf > 0) MESH_LAUNCH(k_topo_shared_corners, nf, st, faces, faces_int64, nf, face_label, vertex_label, keys_out, capacity, count_out);
    return NKSR_OK;
}

extern "C" int nksr_topo_count_shared(const uint64_t* keys_sorted, int64_t m, int64_t n_comp, int64_t* counts, void* stream) {
    if (m < 0 || n_comp < 0) return nksr_set_error(NKSR_ERR_ARG, "topo count shared: negative size");
    if (m == 0) return NKSR_OK;
    if (!keys_sorted || !counts) return nksr_set_error(NKSR_ERR_ARG, "topo count shared: NULL arrays");
    MESH_LAUNCH(k_topo_count_shared, m, (hipStream_t)stream, keys_sorted, m, n_comp, counts);
    return NKSR_OK;
}

extern "C" int nksr_topo_component_boxes(const float* v, int64_t nv, const void* faces, int faces_int64, int64_t nf, const int32_t* face_label,
                                         int64_t n_comp, float* box_out, void* stream) {
    int rc = mesh_check_sizes("topo component boxes", nv, nf);
    if (rc) return rc;
    if (n_comp < 0) return nksr_set_error(NKSR_ERR_ARG, "topo component boxes: negative size");
    if (n_comp == 0) return NKSR_OK;
    if (!box_out || (nf > 0 && (!v || !faces || !face_label))) return nksr_set_error(NKSR_ERR_ARG, "topo component boxes: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    MESH_LAUNCH(k_topo_box_init, n_comp * 6, st, (uint32_t*)box_out, n_comp);
    if (nf > 0) MESH_LAUNCH(k_topo_box_faces, nf, st, v, faces, faces_int64, nf, face_label, n_comp, (uint32_t*)box_out);
    MESH_LAUNCH(k_topo_box_decode, n_comp * 6, st, (uint32_t*)box_out, n_comp);
    return NKSR_OK;
}

extern "C" int nksr_topo_compact_mark(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint8_t* face_keep, int32_t* face_flags_out,
                                      int32_t* vertex_flags_out, void* stream) {
    int rc = mesh_check_sizes("topo compact mark", nv, nf);
    if (rc) return rc;
    if (!face_flags_out || !vertex_flags_out || (nf > 0 && (!faces || !face_keep))) return nksr_set_error(NKSR_ERR_ARG, "topo compact mark: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(vertex_flags_out, 0, sizeof(int32_t) * (size_t)(nv + 1), st));
    if (nf == 0) { NKSR_CHECK_HIP(hipMemsetAsync(face_flags_out, 0, sizeof(int32_t), st)); return NKSR_OK; }
    MESH_LAUNCH(k_topo_mark, nf, st, faces, faces_int64, nf, nv, face_keep, face_flags_out, vertex_flags_out);
    return NKSR_OK;
}

extern "C" int nksr_topo_compact_faces(const void* faces, int faces_int64, int64_t nf, int64_t nv, const int32_t* face_flags, const int32_t* face_offsets,
                                       const int32_t* vertex_flags, const int32_t* vertex_offsets, void* faces_out, int64_t* vertex_map_out,
                                       void* stream) {
    int rc = mesh_check_sizes("topo compact faces", nv, nf);
    if (rc) return rc;
    if ((nf > 0 && (!faces || !face_flags || !face_offsets)) || (nv > 0 && (!vertex_flags || !vertex_offsets || !vertex_map_out)))
        return nksr_set_error(NKSR_ERR_ARG, "topo compact faces: NULL arrays");
    const int64_t n = nf > nv ? nf : nv;
    if (n > 0)
        MESH_LAUNCH(k_topo_renumber, n, (hipStream_t)stream, faces, faces_int64, nf, nv, face_flags, face_offsets, vertex_flags, vertex_offsets, faces_out,
                  vertex_map_out);
    return NKSR_OK;
}
