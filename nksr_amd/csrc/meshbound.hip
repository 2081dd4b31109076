// Mesh boundary loops and hole filling (nksr_amd/mesh_boundary.py: MeshBoundary; layouts in include/nksr_hip.h):
//   k_bd_flags          flag the half-edges whose unique edge is of class NKSR_TOPO_BOUNDARY (their scan is the boundary id)
//   k_bd_list           half-edge, tail, head and face of every boundary id
//   k_bd_successor      the umbrella walk about the head (successor) and about the tail (predecessor) of every boundary half-edge
//   k_bd_loop_sizes     the loop of every boundary half-edge, the representatives, edge and vertex counts per loop
//   k_bd_terms          ordered half-edge and vertex lists; the length, area and centroid terms at (loop offset + rank)
//   k_bd_box_*          loop boxes by 64-bit order-preserving integer min / max
//   k_bd_fill           the faces that close the kept loops (centroid star or fan), k_bd_fill_vertices the new vertices and colours
// The ranking between the successor and the sizes is nksr_chain_rank (csrc/meshslice.hip) as it is.  No floating-point atomic: ids are
// scans plus offsets, every write has one writer, the sums are by-key scans (nksr_inclusive_sum_by_key_f64); the one atomic is the
// integer min / max of the boxes, whose result does not depend on the order.  Every array repeats bit for bit.  All kernels are one lane
// per item and bound by their gathers.
#include "common.h"
#include "mesh_dev.h"

// The terms are stated operation by operation: products and sums round separately, so numpy gives the same bits.
#pragma clang fp contract(off)

// ---- 1. boundary half-edges --------------------------------------------------------------------------------------------------------
// (an invalid face's half-edges have no unique edge: halfedge_edge = -1)
__global__ void __launch_bounds__(MESH_BLOCK) k_bd_flags(const int32_t* __restrict__ he_edge, const uint8_t* __restrict__ edge_class, int64_t nh,
                                                         int64_t ne, int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (h == 0) flags[nh] = 0;
    if (h >= nh) return;
    const int32_t e = he_edge[h];
    flags[h] = e >= 0 && e < ne && edge_class[e] == NKSR_TOPO_BOUNDARY ? 1 : 0;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_bd_list(const void* faces, int is64, int64_t nh, const int32_t* __restrict__ flags,
                                                        const int32_t* __restrict__ bid, int64_t nb, int32_t* __restrict__ halfedge,
                                                        int32_t* __restrict__ tail, int32_t* __restrict__ head, int32_t* __restrict__ face) {
    const int64_t h = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (h >= nh || !flags[h]) return;
    const int64_t b = bid[h];
    if (b < 0 || b >= nb) return;
    const int64_t f = h / 3, k = h - f * 3;
    halfedge[b] = (int32_t)h;
    tail[b] = (int32_t)mesh_face_index(faces, is64, f * 3 + k);
    head[b] = (int32_t)mesh_face_index(faces, is64, f * 3 + (k + 1) % 3);
    face[b] = (int32_t)f;
}

// ---- 2. successor and predecessor --------------------------------------------------------------------------------------------------
// Rotation about the head b of the boundary half-edge (a -> b) of face f: the next half-edge of f is (b -> c).  BOUNDARY: it is the
// successor.  INTERIOR: its twin (c -> b) lies in face_adj; the half-edge after the twin is (b -> d), and so on.  Any other class: none.
// The map incoming -> twin(next(incoming)) is injective on the half-edges that run into b and a boundary half-edge has no pre-image, so
// the orbit is a simple path of at most valence(b) steps: the loop ends by itself.  The predecessor is the mirror image about the tail.
__device__ __forceinline__ int32_t bd_walk(const void* faces, int is64, const int32_t* __restrict__ he_edge, const uint8_t* __restrict__ edge_class,
                                           const int32_t* __restrict__ face_adj, const int32_t* __restrict__ bid, int64_t nf, int64_t h0,
                                           const bool forward) {
    int64_t f = h0 / 3;
    int k = (int)(h0 - f * 3);
    // forward: pivot = the head, step to the next half-edge of the face; backward: pivot = the tail, step to the previous one
    const int64_t pivot = mesh_face_index(faces, is64, f * 3 + (forward ? (k + 1) % 3 : k));
    for (;;) {
        k = forward ? (k + 1) % 3 : (k + 2) % 3;
        const int64_t h = f * 3 + k;
        const int32_t e = he_edge[h];
        if (e < 0) return -1;
        const uint8_t cls = edge_class[e];
        if (cls == NKSR_TOPO_BOUNDARY) return bid[h];
        if (cls != NKSR_TOPO_INTERIOR) return -1;
        const int64_t g = face_adj[h];
        if (g < 0 || g >= nf) return -1;
        // the other end of the half-edge just crossed, and the corner of g where the twin sits
        const int64_t other = mesh_face_index(faces, is64, f * 3 + (forward ? (k + 1) % 3 : k));
        int j = -1;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int64_t a = mesh_face_index(faces, is64, g * 3 + q), b = mesh_face_index(faces, is64, g * 3 + (q + 1) % 3);
            if (forward ? (a == other && b == pivot) : (a == pivot && b == other)) j = q;
        }
        if (j < 0) return -1;                           // (never on an INTERIOR edge: its two half-edges run in opposite directions)
        f = g;
        k = j;
    }
}

__global__ void __launch_bounds__(MESH_BLOCK) k_bd_successor(const void* faces, int is64, int64_t nf, const int32_t* __restrict__ he_edge,
                                                             const uint8_t* __restrict__ edge_class, const int32_t* __restrict__ face_adj,
                                                             const int32_t* __restrict__ bid, const int32_t* __restrict__ halfedge, int64_t nb,
                                                             int32_t* __restrict__ succ, int32_t* __restrict__ pred) {
    const int64_t b = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (b >= nb) return;
    const int64_t h = halfedge[b];
    if (h < 0 || h >= nf * 3) { succ[b] = -1; pred[b] = -1; return; }
    succ[b] = bd_walk(faces, is64, he_edge, edge_class, face_adj, bid, nf, h, true);
    pred[b] = bd_walk(faces, is64, he_edge, edge_class, face_adj, bid, nf, h, false);
}

// ---- 3. loops ------------------------------------------------------------------------------------------------------------------------
// loop = the dense id of the representative (ids ascend by representative); the representative writes itself into the list, the last
// half-edge of a loop (no successor, or the successor is the representative) writes the sizes
__global__ void __launch_bounds__(MESH_BLOCK) k_bd_loop_sizes(const int32_t* __restrict__ rep, const int32_t* __restrict__ rank,
                                                              const uint8_t* __restrict__ cyclic, const int32_t* __restrict__ succ, int64_t nb,
                                                              const int32_t* __restrict__ dense, int64_t nl, int32_t* __restrict__ loop_of,
                                                              int32_t* __restrict__ loop_rep, int32_t* __restrict__ n_edges,
                                                              int32_t* __restrict__ n_pts, uint8_t* __restrict__ closed) {
    const int64_t b = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (b == 0) { n_edges[nl] = 0; n_pts[nl] = 0; }
    if (b >= nb) return;
    const int32_t r = rep[b], l = dense[r];
    loop_of[b] = l;
    if (l < 0 || l >= nl) return;
    if (r == (int32_t)b) loop_rep[l] = r;
    const int32_t nx = succ[b];
    if (nx < 0 || nx == r) {
        const int32_t m = rank[b] + 1;
        n_edges[l] = m;
        n_pts[l] = cyclic[b] ? m : m + 1;
        closed[l] = cyclic[b];
    }
}

// ---- 4. measures ---------------------------------------------------------------------------------------------------------------------
// terms [7, nb] at column (edge offset + rank): 0 the length w, 1..3 the area vector term 0.5 (p - p0) x (q - p0) (0 on an open chain),
// 4..6 the centroid term w * 0.5 ((p - p0) + (q - p0)); p the tail, q the head, p0 the representative's tail
__global__ void __launch_bounds__(MESH_BLOCK) k_bd_terms(const void* v, int v_f64, int64_t nv, const int32_t* __restrict__ halfedge, const int32_t* __restrict__ tail,
                                                         const int32_t* __restrict__ head, const int32_t* __restrict__ rank,
                                                         const uint8_t* __restrict__ cyclic, const int32_t* __restrict__ succ, int64_t nb,
                                                         const int32_t* __restrict__ loop_of, const int32_t* __restrict__ loop_rep,
                                                         const int32_t* __restrict__ edge_offset, const int32_t* __restrict__ pt_offset, int64_t nl,
                                                         int32_t* __restrict__ loop_halfedges, int32_t* __restrict__ loop_vertices,
                                                         uint64_t* __restrict__ term_key, double* __restrict__ terms) {
    const int64_t b = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (b >= nb) return;
    const int32_t l = loop_of[b], r = rank[b];
    if (l < 0 || l >= nl) return;
    const int64_t pos = (int64_t)edge_offset[l] + r, at = (int64_t)pt_offset[l] + r;
    if (pos < 0 || pos >= nb || at < 0 || at + 1 > nb + nl) return;
    const int32_t it = tail[b], ih = head[b], r0 = loop_rep[l];
    if (r0 < 0 || r0 >= nb || it < 0 || it >= nv || ih < 0 || ih >= nv) return;
    const int32_t i0 = tail[r0];
    if (i0 < 0 || i0 >= nv) return;
    loop_halfedges[pos] = halfedge[b];
    loop_vertices[at] = it;
    if (!cyclic[b] && succ[b] < 0) loop_vertices[at + 1] = ih;
    const gm_vec3 p0 = gm_pos(v, v_f64, i0);
    const gm_vec3 p = gm_pos(v, v_f64, it), q = gm_pos(v, v_f64, ih);
    const gm_vec3 a = gm_sub(p, p0), c = gm_sub(q, p0);
    const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const double w = sqrt(dx * dx + dy * dy + dz * dz);
    term_key[pos] = (uint64_t)l;
    terms[pos] = w;
    const bool cyc = cyclic[b] != 0;
    terms[nb + pos] = cyc ? 0.5 * (a.y * c.z - a.z * c.y) : 0.0;
    terms[2 * nb + pos] = cyc ? 0.5 * (a.z * c.x - a.x * c.z) : 0.0;
    terms[3 * nb + pos] = cyc ? 0.5 * (a.x * c.y - a.y * c.x) : 0.0;
    terms[4 * nb + pos] = w * (0.5 * (a.x + c.x));
    terms[5 * nb + pos] = w * (0.5 * (a.y + c.y));
    terms[6 * nb + pos] = w * (0.5 * (a.z + c.z));
}

// boxes: doubles as order-preserving 64-bit integers (-0 counts as +0)
__device__ __forceinline__ unsigned long long bd_ordered(double x) {
    const double y = x == 0.0 ? 0.0 : x;
    const unsigned long long u = (unsigned long long)__double_as_longlong(y);
    return u ^ ((u >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}
__device__ __forceinline__ double bd_unordered(unsigned long long u) {
    return __longlong_as_double((long long)(u & 0x8000000000000000ull ? u & 0x7FFFFFFFFFFFFFFFull : ~u));
}

__global__ void __launch_bounds__(MESH_BLOCK) k_bd_box_init(unsigned long long* __restrict__ work, int64_t n6) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n6) work[i] = i % 6 < 3 ? 0xFFFFFFFFFFFFFFFFull : 0ull;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_bd_box_reduce(const void* v, int v_f64, int64_t nv, const int32_t* __restrict__ tail, const int32_t* __restrict__ head,
                                                              const int32_t* __restrict__ loop_of, int64_t nb, int64_t nl,
                                                              unsigned long long* __restrict__ work) {
    const int64_t b = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (b >= nb) return;
    const int64_t l = loop_of[b];
    const int64_t it = tail[b], ih = head[b];
    if (l < 0 || l >= nl || it < 0 || it >= nv || ih < 0 || ih >= nv) return;
    const gm_vec3 p = gm_pos(v, v_f64, it), q = gm_pos(v, v_f64, ih);
    const double lo[3] = {fmin(p.x, q.x), fmin(p.y, q.y), fmin(p.z, q.z)}, hi[3] = {fmax(p.x, q.x), fmax(p.y, q.y), fmax(p.z, q.z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(work + l * 6 + a, bd_ordered(lo[a]));
        atomicMax(work + l * 6 + 3 + a, bd_ordered(hi[a]));
    }
}

__global__ void __launch_bounds__(MESH_BLOCK) k_bd_box_decode(const unsigned long long* __restrict__ work, int64_t n6, double* __restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n6) box[i] = bd_unordered(work[i]);
}

// ---- 5. fill -------------------------------------------------------------------------------------------------------------------------
// One lane per boundary half-edge (a -> b) of rank r in a kept loop of m edges.  'centroid' (method 0): new face face_offset[l] + r =
// (b, a, nv + kept_rank[l]).  'fan' (method 1): for 1 <= r <= m - 2 new face face_offset[l] + r - 1 = (b, a, p0).  Both wind against the
// boundary half-edge.
__device__ __forceinline__ void bd_store_face(void* out, int is64, int64_t at, int64_t a, int64_t b, int64_t c) {
    if (is64) { int64_t* o = (int64_t*)out + at * 3; o[0] = a; o[1] = b; o[2] = c; }
    else { int32_t* o = (int32_t*)out + at * 3; o[0] = (int32_t)a; o[1] = (int32_t)b; o[2] = (int32_t)c; }
}

__global__ void __launch_bounds__(MESH_BLOCK) k_bd_fill(const int32_t* __restrict__ tail, const int32_t* __restrict__ head, const int32_t* __restrict__ rank,
                                                        const int32_t* __restrict__ loop_of, int64_t nb, const int32_t* __restrict__ loop_rep,
                                                        const int32_t* __restrict__ loop_edges, const uint8_t* __restrict__ keep,
                                                        const int32_t* __restrict__ kept_rank, const int32_t* __restrict__ face_offset, int64_t nl,
                                                        int method, int64_t nv, int64_t n_new, void* faces_out, int is64,
                                                        int32_t* __restrict__ face_loop) {
    const int64_t b = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (b >= nb) return;
    const int32_t l = loop_of[b];
    if (l < 0 || l >= nl || !keep[l]) return;
    const int32_t r = rank[b], m = loop_edges[l];
    int64_t at, apex;
    if (method == 0) {
        at = (int64_t)face_offset[l] + r;
        apex = nv + kept_rank[l];
    } else {
        if (r < 1 || r > m - 2) return;
        at = (int64_t)face_offset[l] + r - 1;
        const int32_t r0 = loop_rep[l];
        if (r0 < 0 || r0 >= nb) return;
        apex = tail[r0];
    }
    if (at < 0 || at >= n_new) return;
    bd_store_face(faces_out, is64, at, head[b], tail[b], apex);
    face_loop[at] = l;
}

// lane (kept loop, channel c): c < 3 the new vertex = the loop's centroid cast once; c >= 3 the mean of colour channel c - 3 over the
// loop's vertices, summed in fp64 in rank order
__global__ void __launch_bounds__(MESH_BLOCK) k_bd_fill_vertices(const double* __restrict__ centroid, const int32_t* __restrict__ pt_offset,
                                                                 const int32_t* __restrict__ loop_vertices, const int32_t* __restrict__ loop_edges,
                                                                 const uint8_t* __restrict__ keep, const int32_t* __restrict__ kept_rank, int64_t nl,
                                                                 int64_t n_kept, const void* colors, int c_f64, int64_t channels, int64_t nv,
                                                                 void* v_out, int v_f64, double* __restrict__ mean_out) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int64_t per = 3 + channels;
    if (i >= nl * per) return;
    const int64_t l = i / per, c = i - l * per;
    if (!keep[l]) return;
    const int64_t j = kept_rank[l];
    if (j < 0 || j >= n_kept) return;
    if (c < 3) {
        const double x = centroid[l * 3 + c];
        if (v_f64) ((double*)v_out)[j * 3 + c] = x;
        else ((float*)v_out)[j * 3 + c] = (float)x;
        return;
    }
    const int64_t ch = c - 3, s = pt_offset[l], m = loop_edges[l];
    double sum = 0.0;
    for (int64_t q = 0; q < m; ++q) {
        const int64_t vi = loop_vertices[s + q];
        if (vi < 0 || vi >= nv) continue;
        sum += c_f64 ? ((const double*)colors)[vi * channels + ch] : (double)((const float*)colors)[vi * channels + ch];
    }
    mean_out[j * channels + ch] = sum / (double)m;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
static int bd_check_boundary(const char* who, int64_t nb, int64_t nf) {
    if (nb < 0 || nb > 3 * nf) return nksr_set_error(NKSR_ERR_ARG, "%s: n_boundary=%lld of %lld faces", who, (long long)nb, (long long)nf);
    return NKSR_OK;
}

static int bd_check_loops(const char* who, int64_t nl, int64_t nb) {
    if (nb < 0 || nb >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: n_boundary=%lld outside [0, 2^31)", who, (long long)nb);
    if (nl < 0 || nl > nb) return nksr_set_error(NKSR_ERR_ARG, "%s: %lld loops of %lld boundary half-edges", who, (long long)nl, (long long)nb);
    return NKSR_OK;
}

extern "C" int nksr_bnd_flags(const int32_t* halfedge_edge, const uint8_t* edge_class, int64_t nf, int64_t n_edges, int32_t* flags_out, void* stream) {
    int rc = mesh_check_sizes("boundary flags", 0, nf);
    if (rc) return rc;
    if (n_edges < 0 || n_edges > 3 * nf) return nksr_set_error(NKSR_ERR_ARG, "boundary flags: n_edges=%lld of %lld faces", (long long)n_edges, (long long)nf);
    if (!flags_out || (nf > 0 && !halfedge_edge) || (n_edges > 0 && !edge_class)) return nksr_set_error(NKSR_ERR_ARG, "boundary flags: NULL arrays");
    MESH_LAUNCH(k_bd_flags, nf > 0 ? 3 * nf : 1, (hipStream_t)stream, halfedge_edge, edge_class, 3 * nf, n_edges, flags_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_list(const void* faces, int faces_int64, int64_t nf, const int32_t* flags, const int32_t* boundary_of, int64_t n_boundary,
                             int32_t* halfedge_out, int32_t* tail_out, int32_t* head_out, int32_t* face_out, void* stream) {
    int rc = mesh_check_sizes("boundary list", 0, nf);
    if (rc) return rc;
    if ((rc = bd_check_boundary("boundary list", n_boundary, nf))) return rc;
    if (n_boundary == 0) return NKSR_OK;
    if (!faces || !flags || !boundary_of || !halfedge_out || !tail_out || !head_out || !face_out)
        return nksr_set_error(NKSR_ERR_ARG, "boundary list: NULL arrays");
    MESH_LAUNCH(k_bd_list, 3 * nf, (hipStream_t)stream, faces, faces_int64, 3 * nf, flags, boundary_of, n_boundary, halfedge_out, tail_out, head_out,
                face_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_successor(const void* faces, int faces_int64, int64_t nf, const int32_t* halfedge_edge, const uint8_t* edge_class,
                                  const int32_t* face_adj, const int32_t* boundary_of, const int32_t* halfedge, int64_t n_boundary, int32_t* succ_out,
                                  int32_t* pred_out, void* stream) {
    int rc = mesh_check_sizes("boundary successor", 0, nf);
    if (rc) return rc;
    if ((rc = bd_check_boundary("boundary successor", n_boundary, nf))) return rc;
    if (n_boundary == 0) return NKSR_OK;
    if (!faces || !halfedge_edge || !edge_class || !face_adj || !boundary_of || !halfedge || !succ_out || !pred_out)
        return nksr_set_error(NKSR_ERR_ARG, "boundary successor: NULL arrays");
    MESH_LAUNCH(k_bd_successor, n_boundary, (hipStream_t)stream, faces, faces_int64, nf, halfedge_edge, edge_class, face_adj, boundary_of, halfedge,
                n_boundary, succ_out, pred_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_loop_sizes(const int32_t* rep, const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_boundary,
                                   const int32_t* rep_dense, int64_t n_loops, int32_t* boundary_loop_out, int32_t* loop_rep_out, int32_t* loop_edges_out,
                                   int32_t* loop_points_out, uint8_t* closed_out, void* stream) {
    int rc = bd_check_loops("boundary loop sizes", n_loops, n_boundary);
    if (rc) return rc;
    if (!loop_edges_out || !loop_points_out) return nksr_set_error(NKSR_ERR_ARG, "boundary loop sizes: NULL arrays");
    if (n_boundary > 0 && (!rep || !rank || !cyclic || !succ || !rep_dense || !boundary_loop_out || !loop_rep_out || !closed_out))
        return nksr_set_error(NKSR_ERR_ARG, "boundary loop sizes: NULL arrays");
    MESH_LAUNCH(k_bd_loop_sizes, n_boundary > 0 ? n_boundary : 1, (hipStream_t)stream, rep, rank, cyclic, succ, n_boundary, rep_dense, n_loops,
                boundary_loop_out, loop_rep_out, loop_edges_out, loop_points_out, closed_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_terms(const void* v, int v_float64, int64_t nv, const int32_t* halfedge, const int32_t* tail, const int32_t* head,
                              const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_boundary, const int32_t* boundary_loop,
                              const int32_t* loop_rep, const int32_t* edge_offset, const int32_t* point_offset, int64_t n_loops,
                              int32_t* loop_halfedges_out, int32_t* loop_vertices_out, uint64_t* term_key_out, double* terms_out, void* stream) {
    int rc = mesh_check_sizes("boundary terms", nv, 0);
    if (rc) return rc;
    if ((rc = bd_check_loops("boundary terms", n_loops, n_boundary))) return rc;
    if (n_boundary == 0) return NKSR_OK;
    if (!v || !halfedge || !tail || !head || !rank || !cyclic || !succ || !boundary_loop || !loop_rep || !edge_offset || !point_offset ||
        !loop_halfedges_out || !loop_vertices_out || !term_key_out || !terms_out)
        return nksr_set_error(NKSR_ERR_ARG, "boundary terms: NULL arrays");
    MESH_LAUNCH(k_bd_terms, n_boundary, (hipStream_t)stream, v, v_float64, nv, halfedge, tail, head, rank, cyclic, succ, n_boundary, boundary_loop, loop_rep,
                edge_offset, point_offset, n_loops, loop_halfedges_out, loop_vertices_out, term_key_out, terms_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_boxes(const void* v, int v_float64, int64_t nv, const int32_t* tail, const int32_t* head, const int32_t* boundary_loop,
                              int64_t n_boundary, int64_t n_loops, uint64_t* work, double* box_out, void* stream) {
    int rc = mesh_check_sizes("boundary boxes", nv, 0);
    if (rc) return rc;
    if ((rc = bd_check_loops("boundary boxes", n_loops, n_boundary))) return rc;
    if (n_loops == 0) return NKSR_OK;
    if (!v || !tail || !head || !boundary_loop || !work || !box_out) return nksr_set_error(NKSR_ERR_ARG, "boundary boxes: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    MESH_LAUNCH(k_bd_box_init, n_loops * 6, st, (unsigned long long*)work, n_loops * 6);
    MESH_LAUNCH(k_bd_box_reduce, n_boundary, st, v, v_float64, nv, tail, head, boundary_loop, n_boundary, n_loops, (unsigned long long*)work);
    MESH_LAUNCH(k_bd_box_decode, n_loops * 6, st, (const unsigned long long*)work, n_loops * 6, box_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_fill(const int32_t* tail, const int32_t* head, const int32_t* rank, const int32_t* boundary_loop, int64_t n_boundary,
                             const int32_t* loop_rep, const int32_t* loop_edges, const uint8_t* keep, const int32_t* kept_rank, const int32_t* face_offset,
                             int64_t n_loops, int method, int64_t nv, int64_t n_new_faces, void* faces_out, int faces_int64, int32_t* face_loop_out,
                             void* stream) {
    int rc = mesh_check_sizes("boundary fill", nv, 0);
    if (rc) return rc;
    if ((rc = bd_check_loops("boundary fill", n_loops, n_boundary))) return rc;
    if (method != 0 && method != 1) return nksr_set_error(NKSR_ERR_ARG, "boundary fill: method=%d, 0 (centroid) or 1 (fan)", method);
    if (n_new_faces < 0 || n_new_faces > n_boundary)
        return nksr_set_error(NKSR_ERR_ARG, "boundary fill: %lld new faces of %lld boundary half-edges", (long long)n_new_faces, (long long)n_boundary);
    if (!faces_int64 && nv + n_loops >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "boundary fill: new vertex ids beyond int32 faces");
    if (n_new_faces == 0) return NKSR_OK;
    if (!tail || !head || !rank || !boundary_loop || !loop_rep || !loop_edges || !keep || !kept_rank || !face_offset || !faces_out || !face_loop_out)
        return nksr_set_error(NKSR_ERR_ARG, "boundary fill: NULL arrays");
    MESH_LAUNCH(k_bd_fill, n_boundary, (hipStream_t)stream, tail, head, rank, boundary_loop, n_boundary, loop_rep, loop_edges, keep, kept_rank, face_offset,
                n_loops, method, nv, n_new_faces, faces_out, faces_int64, face_loop_out);
    return NKSR_OK;
}

extern "C" int nksr_bnd_fill_vertices(const double* loop_centroid, const int32_t* point_offset, const int32_t* loop_vertices, const int32_t* loop_edges,
                                      const uint8_t* keep, const int32_t* kept_rank, int64_t n_loops, int64_t n_kept, const void* colors,
                                      int colors_float64, int64_t channels, int64_t nv, void* v_out, int v_float64, double* color_mean_out,
                                      void* stream) {
    int rc = mesh_check_sizes("boundary fill vertices", nv, 0);
    if (rc) return rc;
    if (n_loops < 0 || n_loops >= (1ll << 31) || n_kept < 0 || n_kept > n_loops)
        return nksr_set_error(NKSR_ERR_ARG, "boundary fill vertices: %lld kept of %lld loops", (long long)n_kept, (long long)n_loops);
    if (channels < 0 || channels > 1024) return nksr_set_error(NKSR_ERR_ARG, "boundary fill vertices: channels=%lld outside [0, 1024]", (long long)channels);
    if (n_kept == 0) return NKSR_OK;
    if (!loop_centroid || !point_offset || !loop_vertices || !loop_edges || !keep || !kept_rank || !v_out || (channels > 0 && (!colors || !color_mean_out)))
        return nksr_set_error(NKSR_ERR_ARG, "boundary fill vertices: NULL arrays");
    MESH_LAUNCH(k_bd_fill_vertices, n_loops * (3 + channels), (hipStream_t)stream, loop_centroid, point_offset, loop_vertices, loop_edges, keep, kept_rank,
                n_loops, n_kept, colors, colors_float64, channels, nv, v_out, v_float64, color_mean_out);
    return NKSR_OK;
}
