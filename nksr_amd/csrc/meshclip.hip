// Mesh clipping (nksr_amd/mesh_clip.py: MeshClipper; layouts in include/nksr_hip.h):
//   k_cl_faces_by_face      every valid face that crosses k planes -> its k + 1 pieces -> 2 k + 1 triangles; one lane per face
//   k_cl_faces_by_piece     the same triangles, one lane per (face, piece)
//   k_cl_attr               vertex attributes at the cut points, t recomputed from the heights as nksr_slice_points computes it
//   k_cl_corner_keys        (label, vertex) keys of the corners of a labelled mesh
//   k_cl_group_faces        the faces in label order with their corners renumbered
// The cut points are the slicer's (csrc/meshslice.hip): this file adds no point and decides no side on its own -- the slab of a corner
// is sl_upper of its height, the search nksr_slice_counts runs.  No atomics: the id of every triangle is face_start (a scan) plus a
// closed form of the three slabs, every write has one writer, so every array repeats bit for bit.
#include "common.h"
#include "mesh_dev.h"
#include "meshslice_dev.h"

// the attributes are stated operation by operation, as the points are
#pragma clang fp contract(off)

// ---- 1. faces ----------------------------------------------------------------------------------------------------------------------
// What a piece is made from: the slabs and ids of the three corners and, per half-edge i (corner i -> corner i + 1), the id its point
// of plane 0 would have: base = nv + point_start[e] - min(slab_i, slab_i+1), so that the point of plane j is base + j.  (min of the
// two slabs IS edge_lo[e] of nksr_slice_counts: sl_upper is monotone, and both run on the same heights and offsets.)
struct cl_face {
    int32_t s0, s1, s2, c0, c1, c2, b0, b1, b2;
};

__device__ __forceinline__ cl_face cl_load_face(const double* __restrict__ h, const void* faces, int is64, int64_t f, const double* o, int32_t np,
                                                const int32_t* __restrict__ he_edge, const int64_t* __restrict__ point_start, int64_t nv) {
    cl_face r;
    const int64_t c0 = mesh_face_index(faces, is64, f * 3), c1 = mesh_face_index(faces, is64, f * 3 + 1), c2 = mesh_face_index(faces, is64, f * 3 + 2);
    r.c0 = (int32_t)c0; r.c1 = (int32_t)c1; r.c2 = (int32_t)c2;
    r.s0 = sl_upper(o, np, h[c0]); r.s1 = sl_upper(o, np, h[c1]); r.s2 = sl_upper(o, np, h[c2]);
    r.b0 = (int32_t)(nv + point_start[he_edge[f * 3]] - min(r.s0, r.s1));
    r.b1 = (int32_t)(nv + point_start[he_edge[f * 3 + 1]] - min(r.s1, r.s2));
    r.b2 = (int32_t)(nv + point_start[he_edge[f * 3 + 2]] - min(r.s2, r.s0));
    return r;
}

// The fan of one piece: its members arrive in walk order; from the third on every member closes a triangle (first, previous, member).
struct cl_fan {
    int32_t first, prev, n;
    int64_t out;
};

__device__ __forceinline__ void cl_push(cl_fan& fan, int32_t m, int32_t f, int32_t s, int32_t* __restrict__ f2, int32_t* __restrict__ source,
                                        int32_t* __restrict__ part) {
    if (fan.n >= 2) {
        f2[fan.out * 3] = fan.first;
        f2[fan.out * 3 + 1] = fan.prev;
        f2[fan.out * 3 + 2] = m;
        source[fan.out] = f;
        part[fan.out] = s;
        ++fan.out;
    }
    if (fan.n == 0) fan.first = m;
    fan.prev = m;
    ++fan.n;
}

// the members of piece s on the half-edge a -> b: the corner a when it lies in slab s, then the points of planes s - 1 and s where the
// half-edge crosses them ([min, max) of the two slabs), in travel order
__device__ __forceinline__ void cl_half_edge(cl_fan& fan, int32_t s, int32_t sa, int32_t sb, int32_t ca, int32_t base, int32_t f,
                                             int32_t* __restrict__ f2, int32_t* __restrict__ source, int32_t* __restrict__ part) {
    if (sa == s) cl_push(fan, ca, f, s, f2, source, part);
    const int32_t lo = min(sa, sb), hi = max(sa, sb);
    const int32_t j1 = sa < sb ? s - 1 : s, j2 = sa < sb ? s : s - 1;
    if (j1 >= lo && j1 < hi) cl_push(fan, base + j1, f, s, f2, source, part);
    if (j2 >= lo && j2 < hi) cl_push(fan, base + j2, f, s, f2, source, part);
}

// piece s of face f, its triangles from id ``out`` on
__device__ __forceinline__ void cl_piece(const cl_face& a, int32_t s, int32_t f, int64_t out, int32_t* __restrict__ f2,
                                         int32_t* __restrict__ source, int32_t* __restrict__ part) {
    cl_fan fan = {0, 0, 0, out};
    cl_half_edge(fan, s, a.s0, a.s1, a.c0, a.b0, f, f2, source, part);
    cl_half_edge(fan, s, a.s1, a.s2, a.c1, a.b1, f, f2, source, part);
    cl_half_edge(fan, s, a.s2, a.s0, a.c2, a.b2, f, f2, source, part);
}

// the triangles of the pieces before piece s: the corners below slab s plus, for s > smin, 2 (s - smin) - 2 -- the sum over the earlier
// pieces of (corners + 2 [s' > smin] + 2 [s' < smax] - 2), every earlier piece lying below smax
__device__ __forceinline__ int64_t cl_triangles_before(const cl_face& a, int32_t smin, int32_t s) {
    if (s == smin) return 0;
    return (int64_t)(a.s0 < s) + (a.s1 < s) + (a.s2 < s) + 2 * (int64_t)(s - smin) - 2;
}

__device__ __forceinline__ const double* cl_stage_offsets(double* s_off, const double* __restrict__ offsets, int32_t np, bool lds) {
    if (!lds) return offsets;
    for (int32_t k = threadIdx.x; k < np; k += MESH_BLOCK) s_off[k] = offsets[k];
    __syncthreads();
    return s_off;
}

template <bool LDS>
__global__ void __launch_bounds__(MESH_BLOCK) k_cl_faces_by_face(const double* __restrict__ h, int64_t nv, const void* faces, int is64, int64_t nf,
                                                                 const uint8_t* __restrict__ face_valid, const int32_t* __restrict__ he_edge,
                                                                 const int64_t* __restrict__ point_start, const double* __restrict__ offsets,
                                                                 int32_t np, const int64_t* __restrict__ face_start, int32_t* __restrict__ f2,
                                                                 int32_t* __restrict__ source, int32_t* __restrict__ part) {
    __shared__ double s_off[LDS ? SL_LDS_OFFSETS : 1];
    const double* o = cl_stage_offsets(s_off, offsets, np, LDS);
    const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f >= nf || !face_valid[f]) return;
    const cl_face a = cl_load_face(h, faces, is64, f, o, np, he_edge, point_start, nv);
    const int32_t smin = min(a.s0, min(a.s1, a.s2)), smax = max(a.s0, max(a.s1, a.s2));
    const int64_t out = face_start[f];
    for (int32_t s = smin; s <= smax; ++s) cl_piece(a, s, (int32_t)f, out + cl_triangles_before(a, smin, s), f2, source, part);
}

// lane i: piece i; its face is the last one whose piece_start is <= i (an invalid face has no piece and is never found)
template <bool LDS>
__global__ void __launch_bounds__(MESH_BLOCK) k_cl_faces_by_piece(const double* __restrict__ h, int64_t nv, const void* faces, int is64, int64_t nf,
                                                                  const int32_t* __restrict__ he_edge, const int64_t* __restrict__ point_start,
                                                                  const double* __restrict__ offsets, int32_t np,
                                                                  const int64_t* __restrict__ face_start, const int64_t* __restrict__ piece_start,
                                                                  int64_t n_pieces, int32_t* __restrict__ f2, int32_t* __restrict__ source,
                                                                  int32_t* __restrict__ part) {
    __shared__ double s_off[LDS ? SL_LDS_OFFSETS : 1];
    const double* o = cl_stage_offsets(s_off, offsets, np, LDS);
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_pieces) return;
    int64_t lo = 0, hi = nf;                            // the first face with piece_start > i, minus one
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (piece_start[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    const int64_t f = lo - 1;                           // (piece_start[0] = 0 <= i: f >= 0; i < piece_start[nf]: f < nf)
    const cl_face a = cl_load_face(h, faces, is64, f, o, np, he_edge, point_start, nv);
    const int32_t smin = min(a.s0, min(a.s1, a.s2));
    const int32_t s = smin + (int32_t)(i - piece_start[f]);
    cl_piece(a, s, (int32_t)f, face_start[f] + cl_triangles_before(a, smin, s), f2, source, part);
}

// ---- 2. attributes -----------------------------------------------------------------------------------------------------------------
#define CL_ATTR_GROUP 4             // channels per lane

__global__ void __launch_bounds__(MESH_BLOCK) k_cl_attr(const void* attr, int attr_f64, int64_t channels, const double* __restrict__ h,
                                                        const int32_t* __restrict__ edges, const double* __restrict__ offsets,
                                                        const int32_t* __restrict__ point_edge, const int32_t* __restrict__ point_plane,
                                                        int64_t n_points, int64_t groups, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_points * groups) return;
    const int64_t p = i / groups, c0 = (i - p * groups) * CL_ATTR_GROUP;
    const int64_t e = point_edge[p];
    const int64_t ia = edges[e * 2], ib = edges[e * 2 + 1];
    const double ha = h[ia], hb = h[ib];
    const double t = (offsets[point_plane[p]] - ha) / (hb - ha);
    const int64_t c1 = c0 + CL_ATTR_GROUP < channels ? c0 + CL_ATTR_GROUP : channels;
    for (int64_t c = c0; c < c1; ++c) {
        const double a = attr_f64 ? ((const double*)attr)[ia * channels + c] : (double)((const float*)attr)[ia * channels + c];
        const double b = attr_f64 ? ((const double*)attr)[ib * channels + c] : (double)((const float*)attr)[ib * channels + c];
        out[p * channels + c] = a + t * (b - a);
    }
}

// ---- 3. grouping by label ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_cl_corner_keys(const int32_t* __restrict__ f2, const int32_t* __restrict__ labels, int64_t n_corners,
                                                               uint64_t* __restrict__ keys, uint32_t* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_corners) return;
    keys[i] = ((uint64_t)(uint32_t)labels[i / 3] << 32) | (uint64_t)(uint32_t)f2[i];
    ids[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_cl_group_faces(const int32_t* __restrict__ order, const int32_t* __restrict__ corner_vertex, int64_t nf,
                                                               int32_t* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (q >= nf) return;
    const int64_t src = order[q];
    out[q * 3] = corner_vertex[src * 3];
    out[q * 3 + 1] = corner_vertex[src * 3 + 1];
    out[q * 3 + 2] = corner_vertex[src * 3 + 2];
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
static int cl_check_count(const char* who, const char* what, int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: %s=%lld outside [0, 2^31)", who, what, (long long)n);
    return NKSR_OK;
}

extern "C" int nksr_clip_faces(const double* height, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint8_t* face_valid,
                               const int32_t* halfedge_edge, const int64_t* point_start, int64_t n_points, const double* offsets, int64_t n_planes,
                               const int64_t* face_start, const int64_t* piece_start, int64_t n_pieces, int64_t n_faces_out, int by_piece,
                               int32_t* faces_out, int32_t* face_source_out, int32_t* face_part_out, void* stream) {
    int rc = mesh_check_sizes("clip faces", nv, nf);
    if (rc) return rc;
    if ((rc = cl_check_count("clip faces", "n_planes", n_planes))) return rc;
    if ((rc = cl_check_count("clip faces", "n_faces_out", n_faces_out))) return rc;
    if (n_points < 0 || nv + n_points >= (1ll << 31))
        return nksr_set_error(NKSR_ERR_ARG, "clip faces: %lld vertices and %lld points, together at most 2^31 - 1", (long long)nv, (long long)n_points);
    if (n_pieces < 0 || n_pieces > n_faces_out || 2 * n_pieces < n_faces_out)
        return nksr_set_error(NKSR_ERR_ARG, "clip faces: %lld pieces of %lld triangles", (long long)n_pieces, (long long)n_faces_out);
    if (n_faces_out == 0) return NKSR_OK;
    if (nf == 0) return nksr_set_error(NKSR_ERR_ARG, "clip faces: %lld triangles without faces", (long long)n_faces_out);
    if (!height || !faces || !face_valid || !halfedge_edge || !point_start || (n_planes > 0 && !offsets) || !face_start || (by_piece && !piece_start) ||
        !faces_out || !face_source_out || !face_part_out)
        return nksr_set_error(NKSR_ERR_ARG, "clip faces: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    const bool lds = n_planes <= SL_LDS_OFFSETS;
    if (by_piece) {
        if (lds)
            MESH_LAUNCH(k_cl_faces_by_piece<true>, n_pieces, st, height, nv, faces, faces_int64, nf, halfedge_edge, point_start, offsets, (int32_t)n_planes,
                        face_start, piece_start, n_pieces, faces_out, face_source_out, face_part_out);
        else
            MESH_LAUNCH(k_cl_faces_by_piece<false>, n_pieces, st, height, nv, faces, faces_int64, nf, halfedge_edge, point_start, offsets, (int32_t)n_planes,
                        face_start, piece_start, n_pieces, faces_out, face_source_out, face_part_out);
    } else {
        if (lds)
            MESH_LAUNCH(k_cl_faces_by_face<true>, nf, st, height, nv, faces, faces_int64, nf, face_valid, halfedge_edge, point_start, offsets,
                        (int32_t)n_planes, face_start, faces_out, face_source_out, face_part_out);
        else
            MESH_LAUNCH(k_cl_faces_by_face<false>, nf, st, height, nv, faces, faces_int64, nf, face_valid, halfedge_edge, point_start, offsets,
                        (int32_t)n_planes, face_start, faces_out, face_source_out, face_part_out);
    }
    return NKSR_OK;
}

extern "C" int nksr_clip_attr(const void* attr, int attr_float64, int64_t nv, int64_t channels, const double* height, const int32_t* edges,
                              int64_t n_edges, const double* offsets, int64_t n_planes, const int32_t* point_edge, const int32_t* point_plane,
                              int64_t n_points, double* attr_out, void* stream) {
    int rc = mesh_check_sizes("clip attr", nv, 0);
    if (rc) return rc;
    if ((rc = cl_check_count("clip attr", "n_points", n_points))) return rc;
    if ((rc = cl_check_count("clip attr", "channels", channels))) return rc;
    if (n_edges < 0 || n_planes < 0) return nksr_set_error(NKSR_ERR_ARG, "clip attr: negative size");
    if (n_points == 0 || channels == 0) return NKSR_OK;
    if (n_edges == 0 || n_planes == 0) return nksr_set_error(NKSR_ERR_ARG, "clip attr: %lld points without edges or planes", (long long)n_points);
    if (!attr || !height || !edges || !offsets || !point_edge || !point_plane || !attr_out) return nksr_set_error(NKSR_ERR_ARG, "clip attr: NULL arrays");
    const int64_t groups = (channels + CL_ATTR_GROUP - 1) / CL_ATTR_GROUP;
    MESH_LAUNCH(k_cl_attr, n_points * groups, (hipStream_t)stream, attr, attr_float64, channels, height, edges, offsets, point_edge, point_plane, n_points,
                groups, attr_out);
    return NKSR_OK;
}

// (3 nf corner ids in 31 bits: the sorted-run table counts positions in 32)
static int cl_check_group(const char* who, int64_t nf) {
    if (nf < 0 || 3 * nf >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: nf=%lld, 3 nf outside [0, 2^31)", who, (long long)nf);
    return NKSR_OK;
}

extern "C" int nksr_clip_corner_keys(const int32_t* faces, const int32_t* labels, int64_t nf, uint64_t* keys_out, uint32_t* ids_out, void* stream) {
    int rc = cl_check_group("clip corner keys", nf);
    if (rc) return rc;
    if (nf == 0) return NKSR_OK;
    if (!faces || !labels || !keys_out || !ids_out) return nksr_set_error(NKSR_ERR_ARG, "clip corner keys: NULL arrays");
    MESH_LAUNCH(k_cl_corner_keys, 3 * nf, (hipStream_t)stream, faces, labels, 3 * nf, keys_out, ids_out);
    return NKSR_OK;
}

extern "C" int nksr_clip_group_faces(const int32_t* order, const int32_t* corner_vertex, int64_t nf, int32_t* faces_out, void* stream) {
    int rc = cl_check_group("clip group faces", nf);
    if (rc) return rc;
    if (nf == 0) return NKSR_OK;
    if (!order || !corner_vertex || !faces_out) return nksr_set_error(NKSR_ERR_ARG, "clip group faces: NULL arrays");
    MESH_LAUNCH(k_cl_group_faces, nf, (hipStream_t)stream, order, corner_vertex, nf, faces_out);
    return NKSR_OK;
}
