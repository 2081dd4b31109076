// Mesh cross-sections (nksr_amd/mesh_slice.py: MeshSlicer; layouts in include/nksr_hip.h):
//   k_sl_heights        h_v = n . x_v per vertex, fp64, fused multiply-adds in a fixed order
//   k_sl_counts         the planes (lo, count) every face and every unique edge crosses: two binary searches of the sorted offsets
//   k_sl_points         one point per (edge, crossed plane), from the edge's canonical end points
//   k_sl_segments       one segment per (face, crossed plane): tail, head, face, plane, successor and predecessor -- gathers only
//   k_cr_*              list ranking of any predecessor array by pointer doubling (chains and cycles in one sweep)
//   k_sl_poly_*         dense polyline ids, the ordered point lists, the terms of the lengths and the areas
// No atomics anywhere: every id is an exclusive scan plus an offset, every write has one writer, and the floating-point sums are by-key
// scans (nksr_inclusive_sum_by_key_f64), so every array repeats bit for bit.  All kernels are one lane per item and bound by their
// gathers (heights per corner in the face passes, the 16-byte state of the element 2^k steps back in the ranking rounds).
#include "common.h"
#include "mesh_dev.h"
#include "meshslice_dev.h"      // sl_upper, SL_LDS_OFFSETS: shared with csrc/meshclip.hip

// Points, lengths and area terms are stated operation by operation: products and sums round separately, so
// numpy gives the same bits.  The heights alone are fused, by explicit fma().
#pragma clang fp contract(off)

// ---- 1. heights ------------------------------------------------------------------------------------------------------------------
// (a height that is not a number becomes -inf: a vertex without a position lies below every plane, for the faces and the edges alike)
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_heights(const void* v, int v_f64, int64_t nv, double nx, double ny, double nz,
                                                           double* __restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= nv) return;
    const gm_vec3 p = gm_pos(v, v_f64, i);
    const double r = fma(nz, p.z, fma(ny, p.y, nx * p.x));
    h[i] = r == r ? r : -__builtin_huge_val();
}

// ---- 2. plane ranges ---------------------------------------------------------------------------------------------------------------
// lane i: face i (i < nf) and edge i (i < ne).  lo = planes at or below the lower height, count = planes in (lower, upper].
template <bool LDS>
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_counts(const double* __restrict__ h, int64_t nv, const void* faces, int is64, int64_t nf,
                                                          const uint8_t* __restrict__ face_valid, const int32_t* __restrict__ edges, int64_t ne,
                                                          const double* __restrict__ offsets, int32_t np, int32_t* __restrict__ lo_f,
                                                          int64_t* __restrict__ cnt_f, int32_t* __restrict__ lo_e, int64_t* __restrict__ cnt_e) {
    __shared__ double s_off[LDS ? SL_LDS_OFFSETS : 1];
    const double* o = offsets;
    if (LDS) {
        for (int32_t k = threadIdx.x; k < np; k += MESH_BLOCK) s_off[k] = offsets[k];
        __syncthreads();
        o = s_off;
    }
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < nf) {
        int32_t lo = 0, cnt = 0;
        if (face_valid[i]) {
            const double a = h[mesh_face_index(faces, is64, i * 3)], b = h[mesh_face_index(faces, is64, i * 3 + 1)],
                         c = h[mesh_face_index(faces, is64, i * 3 + 2)];
            const double mn = fmin(a, fmin(b, c)), mx = fmax(a, fmax(b, c));
            lo = sl_upper(o, np, mn);
            cnt = sl_upper(o, np, mx) - lo;
        }
        lo_f[i] = lo;
        cnt_f[i] = cnt;
    }
    if (i < ne) {
        const double a = h[edges[i * 2]], b = h[edges[i * 2 + 1]];
        const int32_t lo = sl_upper(o, np, fmin(a, b));
        lo_e[i] = lo;
        cnt_e[i] = sl_upper(o, np, fmax(a, b)) - lo;
    }
    if (i == 0) { cnt_f[nf] = 0; cnt_e[ne] = 0; }
}

// ---- 3. points ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sl_write_point(const void* v, int v_f64, const double* __restrict__ h, const int32_t* __restrict__ edges,
                                               const double* __restrict__ offsets, int64_t e, int32_t j, int64_t id,
                                               double* __restrict__ points, int32_t* __restrict__ point_edge, int32_t* __restrict__ point_plane) {
    const int64_t ia = edges[e * 2], ib = edges[e * 2 + 1];
    const gm_vec3 a = gm_pos(v, v_f64, ia), b = gm_pos(v, v_f64, ib);
    const double ha = h[ia], hb = h[ib];
    const double t = (offsets[j] - ha) / (hb - ha);
    points[id * 3] = a.x + t * (b.x - a.x);
    points[id * 3 + 1] = a.y + t * (b.y - a.y);
    points[id * 3 + 2] = a.z + t * (b.z - a.z);
    point_edge[id] = (int32_t)e;
    point_plane[id] = j;
}

// one lane per edge, looping over its planes
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_points_by_edge(const void* v, int v_f64, const double* __restrict__ h,
                                                                  const int32_t* __restrict__ edges, int64_t ne, const double* __restrict__ offsets,
                                                                  const int32_t* __restrict__ lo_e, const int64_t* __restrict__ point_start,
                                                                  double* __restrict__ points, int32_t* __restrict__ point_edge,
                                                                  int32_t* __restrict__ point_plane) {
    const int64_t e = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (e >= ne) return;
    const int64_t s = point_start[e], n = point_start[e + 1] - s;
    const int32_t lo = lo_e[e];
    for (int64_t k = 0; k < n; ++k) sl_write_point(v, v_f64, h, edges, offsets, e, lo + (int32_t)k, s + k, points, point_edge, point_plane);
}

// one lane per point: its edge is the last one whose point_start is <= the point id
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_points_by_point(const void* v, int v_f64, const double* __restrict__ h,
                                                                   const int32_t* __restrict__ edges, int64_t ne, const double* __restrict__ offsets,
                                                                   const int32_t* __restrict__ lo_e, const int64_t* __restrict__ point_start,
                                                                   int64_t n_points, double* __restrict__ points, int32_t* __restrict__ point_edge,
                                                                   int32_t* __restrict__ point_plane) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_points) return;
    int64_t lo = 0, hi = ne;                            // the first edge with point_start > i, minus one
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (point_start[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    const int64_t e = lo - 1;                           // (point_start[0] = 0 <= i: e >= 0; i < point_start[ne]: e < ne)
    sl_write_point(v, v_f64, h, edges, offsets, e, lo_e[e] + (int32_t)(i - point_start[e]), i, points, point_edge, point_plane);
}

// ---- 4. segments -------------------------------------------------------------------------------------------------------------------
// One lane per face, looping over its planes.  Half-edge k runs corner k -> corner k + 1; for plane j exactly one half-edge goes
// above -> below (it carries the tail) and one below -> above (the head).  The segment of the face across an INTERIOR edge for the same
// plane is seg_start[g] + (j - lo_f[g]): that face crosses every plane the shared edge crosses.
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_segments(const double* __restrict__ h, const void* faces, int is64, int64_t nf,
                                                            const double* __restrict__ offsets, const int32_t* __restrict__ he_edge,
                                                            const uint8_t* __restrict__ edge_class, const int32_t* __restrict__ face_adj,
                                                            const int32_t* __restrict__ lo_f, const int64_t* __restrict__ seg_start,
                                                            const int32_t* __restrict__ lo_e, const int64_t* __restrict__ point_start,
                                                            int32_t* __restrict__ segments, int32_t* __restrict__ seg_face,
                                                            int32_t* __restrict__ seg_plane, int32_t* __restrict__ succ, int32_t* __restrict__ pred) {
    const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const int64_t s0 = seg_start[f], n = seg_start[f + 1] - s0;
    if (n == 0) return;                                 // (an invalid face has no planes)
    const int32_t lo = lo_f[f];
    double hc[3];
    int32_t e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        hc[k] = h[mesh_face_index(faces, is64, f * 3 + k)];
        e[k] = he_edge[f * 3 + k];
    }
    for (int64_t q = 0; q < n; ++q) {
        const int32_t j = lo + (int32_t)q;
        const double o = offsets[j];
        const bool up0 = hc[0] >= o, up1 = hc[1] >= o, up2 = hc[2] >= o;
        // half-edge k goes down when corner k is above and corner k + 1 is not
        const int kd = up0 && !up1 ? 0 : (up1 && !up2 ? 1 : 2);
        const int ku = !up0 && up1 ? 0 : (!up1 && up2 ? 1 : 2);
        const int32_t ed = e[kd], eu = e[ku];
        const int64_t s = s0 + q;
        segments[s * 2] = (int32_t)(point_start[ed] + (j - lo_e[ed]));
        segments[s * 2 + 1] = (int32_t)(point_start[eu] + (j - lo_e[eu]));
        seg_face[s] = (int32_t)f;
        seg_plane[s] = j;
        int32_t nx = -1, pv = -1;
        if (edge_class[eu] == NKSR_TOPO_INTERIOR) {
            const int32_t g = face_adj[f * 3 + ku];
            nx = (int32_t)(seg_start[g] + (j - lo_f[g]));
        }
        if (edge_class[ed] == NKSR_TOPO_INTERIOR) {
            const int32_t g = face_adj[f * 3 + kd];
            pv = (int32_t)(seg_start[g] + (j - lo_f[g]));
        }
        succ[s] = nx;
        pred[s] = pv;
    }
}

// ---- 5. list ranking ---------------------------------------------------------------------------------------------------------------
// State of element s after round k (window = the 2^k elements s, pred(s), pred^2(s), ...):
//   x  the element 2^k steps back, or the chain's first element once the walk has reached it (a first element points at itself)
//   y  the number of steps taken to get there
//   z  the smallest element id in the window, w its distance back from s (the nearest one when the window has wrapped round a cycle)
// After 2^k >= n: an element of an open chain has x = its first element and y = its rank; an element of a cycle never reaches a fixed
// point, its z is the cycle's smallest id and w its distance from it.  Every round reads one buffer and writes the other.
__global__ void __launch_bounds__(MESH_BLOCK) k_cr_init(const int32_t* __restrict__ pred, int64_t n, int4* __restrict__ st) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s >= n) return;
    const int32_t p = pred[s];
    const bool link = p >= 0 && p < n && p != (int32_t)s;
    st[s] = make_int4(link ? p : (int32_t)s, link ? 1 : 0, (int32_t)s, 0);
}

__global__ void __launch_bounds__(MESH_BLOCK) k_cr_round(const int4* __restrict__ in, int4* __restrict__ out, int64_t n, uint32_t step) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s >= n) return;
    int4 a = in[s];
    if (a.x != (int32_t)s) {                            // (a first element is final)
        const int4 b = in[a.x];
        if (b.z < a.z) { a.z = b.z; a.w = (int32_t)(step + (uint32_t)b.w); }     // strict: the nearer copy of the minimum stays
        a.x = b.x;
        a.y += b.y;
    }
    out[s] = a;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_cr_finish(const int4* __restrict__ st, const int32_t* __restrict__ pred, int64_t n,
                                                          int32_t* __restrict__ rep, int32_t* __restrict__ rank, uint8_t* __restrict__ cyclic,
                                                          int32_t* __restrict__ rep_flags) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s == 0) rep_flags[n] = 0;
    if (s >= n) return;
    const int4 a = st[s];
    const int32_t p = pred[a.x];
    const bool open = !(p >= 0 && p < n && p != a.x);   // x has no predecessor: it is the first element of an open chain
    const int32_t r = open ? a.x : a.z;
    rep[s] = r;
    rank[s] = open ? a.y : a.w;
    cyclic[s] = open ? 0 : 1;
    rep_flags[s] = r == (int32_t)s ? 1 : 0;
}

// ---- 6. polylines ------------------------------------------------------------------------------------------------------------------
// the representatives in ascending segment id: list[dense[s]] = s where flags[s]
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_rep_list(const int32_t* __restrict__ flags, const int32_t* __restrict__ dense, int64_t n,
                                                            const int32_t* __restrict__ seg_plane, int32_t* __restrict__ list,
                                                            uint64_t* __restrict__ plane_key) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s >= n || !flags[s]) return;
    list[dense[s]] = (int32_t)s;
    plane_key[dense[s]] = (uint64_t)seg_plane[s];
}

// polyline of every segment; the last segment of a polyline (no successor, or the successor is the representative) writes its size
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_poly_sizes(const int32_t* __restrict__ rep, const int32_t* __restrict__ rank,
                                                              const uint8_t* __restrict__ cyclic, const int32_t* __restrict__ succ, int64_t n,
                                                              const int32_t* __restrict__ dense, const int32_t* __restrict__ poly_of_dense,
                                                              int64_t n_poly, int32_t* __restrict__ seg_poly, int32_t* __restrict__ n_segs,
                                                              int32_t* __restrict__ n_pts, uint8_t* __restrict__ closed) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s == 0) { n_segs[n_poly] = 0; n_pts[n_poly] = 0; }
    if (s >= n) return;
    const int32_t r = rep[s], l = poly_of_dense[dense[r]];
    seg_poly[s] = l;
    const int32_t nx = succ[s];
    if (nx < 0 || nx == r) {
        const int32_t m = rank[s] + 1;
        n_segs[l] = m;
        n_pts[l] = cyclic[s] ? m : m + 1;
        closed[l] = cyclic[s];
    }
}

// polyline_points by (polyline offset + rank); the length and area term of every segment at (segment offset + rank), keyed by polyline
__global__ void __launch_bounds__(MESH_BLOCK) k_sl_poly_fill(const int32_t* __restrict__ segments, const int32_t* __restrict__ rank,
                                                             const uint8_t* __restrict__ cyclic, const int32_t* __restrict__ succ, int64_t n,
                                                             const int32_t* __restrict__ seg_poly, const int32_t* __restrict__ poly_rep,
                                                             const int32_t* __restrict__ seg_offset, const int32_t* __restrict__ pt_offset,
                                                             const double* __restrict__ points, double nx, double ny, double nz,
                                                             int32_t* __restrict__ poly_points, uint64_t* __restrict__ term_key,
                                                             double* __restrict__ len_term, double* __restrict__ area_term) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s >= n) return;
    const int32_t l = seg_poly[s], r = rank[s];
    const int32_t tail = segments[s * 2], head = segments[s * 2 + 1];
    const int64_t at = (int64_t)pt_offset[l] + r;
    poly_points[at] = tail;
    if (!cyclic[s] && succ[s] < 0) poly_points[at + 1] = head;
    const double* p = points + (int64_t)tail * 3;
    const double* q = points + (int64_t)head * 3;
    const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    const int64_t pos = (int64_t)seg_offset[l] + r;
    term_key[pos] = (uint64_t)l;
    len_term[pos] = sqrt(dx * dx + dy * dy + dz * dz);
    double area = 0.0;
    if (cyclic[s]) {
        const double* c = points + (int64_t)segments[(int64_t)poly_rep[l] * 2] * 3;
        const double ax = p[0] - c[0], ay = p[1] - c[1], az = p[2] - c[2];
        const double bx = q[0] - c[0], by = q[1] - c[1], bz = q[2] - c[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        area = 0.5 * (nx * cx + ny * cy + nz * cz);
    }
    area_term[pos] = area;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
static int sl_check_count(const char* who, const char* what, int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: %s=%lld outside [0, 2^31)", who, what, (long long)n);
    return NKSR_OK;
}

static int sl_check_polylines(const char* who, int64_t n_polylines, int64_t n_segments) {
    if (n_polylines < 0 || n_polylines > n_segments)
        return nksr_set_error(NKSR_ERR_ARG, "%s: %lld polylines of %lld segments", who, (long long)n_polylines, (long long)n_segments);
    return NKSR_OK;
}

extern "C" int nksr_slice_heights(const void* v, int v_float64, int64_t nv, const double* normal, double* height_out, void* stream) {
    int rc = mesh_check_sizes("slice heights", nv, 0);
    if (rc) return rc;
    if (!normal || (nv > 0 && (!v || !height_out))) return nksr_set_error(NKSR_ERR_ARG, "slice heights: NULL arrays");
    if (nv > 0) MESH_LAUNCH(k_sl_heights, nv, (hipStream_t)stream, v, v_float64, nv, normal[0], normal[1], normal[2], height_out);
    return NKSR_OK;
}

extern "C" int nksr_slice_counts(const double* height, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint8_t* face_valid,
                                 const int32_t* edges, int64_t n_edges, const double* offsets, int64_t n_planes, int32_t* face_lo_out,
                                 int64_t* face_count_out, int32_t* edge_lo_out, int64_t* edge_count_out, void* stream) {
    int rc = mesh_check_sizes("slice counts", nv, nf);
    if (rc) return rc;
    if ((rc = sl_check_count("slice counts", "n_planes", n_planes))) return rc;
    if (n_edges < 0 || n_edges > 3 * nf) return nksr_set_error(NKSR_ERR_ARG, "slice counts: n_edges=%lld of %lld faces", (long long)n_edges, (long long)nf);
    if (!face_count_out || !edge_count_out || (n_planes > 0 && !offsets) || (nf > 0 && (!height || !faces || !face_valid || !face_lo_out)) ||
        (n_edges > 0 && (!edges || !edge_lo_out)))
        return nksr_set_error(NKSR_ERR_ARG, "slice counts: NULL arrays");
    const int64_t n = (nf > n_edges ? nf : n_edges) > 0 ? (nf > n_edges ? nf : n_edges) : 1;        // (lane 0 closes both count arrays)
    if (n_planes <= SL_LDS_OFFSETS)
        MESH_LAUNCH(k_sl_counts<true>, n, (hipStream_t)stream, height, nv, faces, faces_int64, nf, face_valid, edges, n_edges, offsets,
                    (int32_t)n_planes, face_lo_out, face_count_out, edge_lo_out, edge_count_out);
    else
        MESH_LAUNCH(k_sl_counts<false>, n, (hipStream_t)stream, height, nv, faces, faces_int64, nf, face_valid, edges, n_edges, offsets,
                    (int32_t)n_planes, face_lo_out, face_count_out, edge_lo_out, edge_count_out);
    return NKSR_OK;
}

extern "C" int nksr_slice_points(const void* v, int v_float64, int64_t nv, const double* height, const int32_t* edges, int64_t n_edges,
                                 const double* offsets, int64_t n_planes, const int32_t* edge_lo, const int64_t* point_start, int64_t n_points,
                                 int by_point, double* points_out, int32_t* point_edge_out, int32_t* point_plane_out, void* stream) {
    int rc = mesh_check_sizes("slice points", nv, 0);
    if (rc) return rc;
    if ((rc = sl_check_count("slice points", "n_points", n_points))) return rc;
    if (n_edges < 0 || n_planes < 0) return nksr_set_error(NKSR_ERR_ARG, "slice points: negative size");
    if (n_points == 0) return NKSR_OK;
    if (n_edges == 0 || n_planes == 0) return nksr_set_error(NKSR_ERR_ARG, "slice points: %lld points without edges or planes", (long long)n_points);
    if (!v || !height || !edges || !offsets || !edge_lo || !point_start || !points_out || !point_edge_out || !point_plane_out)
        return nksr_set_error(NKSR_ERR_ARG, "slice points: NULL arrays");
    if (by_point)
        MESH_LAUNCH(k_sl_points_by_point, n_points, (hipStream_t)stream, v, v_float64, height, edges, n_edges, offsets, edge_lo, point_start, n_points,
                    points_out, point_edge_out, point_plane_out);
    else
        MESH_LAUNCH(k_sl_points_by_edge, n_edges, (hipStream_t)stream, v, v_float64, height, edges, n_edges, offsets, edge_lo, point_start, points_out,
                    point_edge_out, point_plane_out);
    return NKSR_OK;
}

extern "C" int nksr_slice_segments(const double* height, int64_t nv, const void* faces, int faces_int64, int64_t nf, const double* offsets,
                                   int64_t n_planes, const int32_t* halfedge_edge, const uint8_t* edge_class, const int32_t* face_adj,
                                   const int32_t* face_lo, const int64_t* seg_start, const int32_t* edge_lo, const int64_t* point_start,
                                   int64_t n_segments, int32_t* segments_out, int32_t* segment_face_out, int32_t* segment_plane_out,
                                   int32_t* succ_out, int32_t* pred_out, void* stream) {
    int rc = mesh_check_sizes("slice segments", nv, nf);
    if (rc) return rc;
    if ((rc = sl_check_count("slice segments", "n_segments", n_segments))) return rc;
    if (n_planes < 0) return nksr_set_error(NKSR_ERR_ARG, "slice segments: negative size");
    if (n_segments == 0) return NKSR_OK;
    if (nf == 0 || n_planes == 0) return nksr_set_error(NKSR_ERR_ARG, "slice segments: %lld segments without faces or planes", (long long)n_segments);
    if (!height || !faces || !offsets || !halfedge_edge || !edge_class || !face_adj || !face_lo || !seg_start || !edge_lo || !point_start ||
        !segments_out || !segment_face_out || !segment_plane_out || !succ_out || !pred_out)
        return nksr_set_error(NKSR_ERR_ARG, "slice segments: NULL arrays");
    MESH_LAUNCH(k_sl_segments, nf, (hipStream_t)stream, height, faces, faces_int64, nf, offsets, halfedge_edge, edge_class, face_adj, face_lo, seg_start,
                edge_lo, point_start, segments_out, segment_face_out, segment_plane_out, succ_out, pred_out);
    return NKSR_OK;
}

extern "C" int64_t nksr_chain_rank_rounds(int64_t n) {
    int64_t r = 0;
    while (r < 62 && (1ll << r) < n) ++r;
    return r + 1;
}

extern "C" int nksr_chain_rank(const int32_t* pred, int64_t n, void* work, int32_t* rep_out, int32_t* rank_out, uint8_t* cyclic_out,
                               int32_t* rep_flags_out, void* stream) {
    int rc = sl_check_count("chain rank", "n", n);
    if (rc) return rc;
    if (!rep_flags_out) return nksr_set_error(NKSR_ERR_ARG, "chain rank: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { NKSR_CHECK_HIP(hipMemsetAsync(rep_flags_out, 0, sizeof(int32_t), st)); return NKSR_OK; }
    if (!pred || !work || !rep_out || !rank_out || !cyclic_out) return nksr_set_error(NKSR_ERR_ARG, "chain rank: NULL arrays");
    if (((uintptr_t)work & 15) != 0) return nksr_set_error(NKSR_ERR_ARG, "chain rank: work must be 16-byte aligned");
    int4* a = (int4*)work;
    int4* b = a + n;
    MESH_LAUNCH(k_cr_init, n, st, pred, n, a);
    const int64_t rounds = nksr_chain_rank_rounds(n);
    for (int64_t k = 0; k < rounds; ++k) {              // queued back to back: nothing is read on the host between rounds
        MESH_LAUNCH(k_cr_round, n, st, (const int4*)a, b, n, (uint32_t)1u << (k < 31 ? k : 31));
        int4* t = a; a = b; b = t;
    }
    MESH_LAUNCH(k_cr_finish, n, st, (const int4*)a, pred, n, rep_out, rank_out, cyclic_out, rep_flags_out);
    return NKSR_OK;
}

extern "C" int nksr_slice_rep_list(const int32_t* rep_flags, const int32_t* rep_dense, int64_t n_segments, const int32_t* segment_plane,
                                   int64_t n_polylines, int32_t* list_out, uint64_t* plane_key_out, void* stream) {
    int rc = sl_check_count("slice rep list", "n_segments", n_segments);
    if (rc) return rc;
    if ((rc = sl_check_polylines("slice rep list", n_polylines, n_segments))) return rc;
    if (n_segments == 0) return NKSR_OK;
    if (!rep_flags || !rep_dense || !segment_plane || (n_polylines > 0 && (!list_out || !plane_key_out)))
        return nksr_set_error(NKSR_ERR_ARG, "slice rep list: NULL arrays");
    MESH_LAUNCH(k_sl_rep_list, n_segments, (hipStream_t)stream, rep_flags, rep_dense, n_segments, segment_plane, list_out, plane_key_out);
    return NKSR_OK;
}

extern "C" int nksr_slice_polyline_sizes(const int32_t* rep, const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_segments,
                                         const int32_t* rep_dense, const int32_t* polyline_of_dense, int64_t n_polylines, int32_t* segment_polyline_out,
                                         int32_t* n_segments_out, int32_t* n_points_out, uint8_t* closed_out, void* stream) {
    int rc = sl_check_count("slice polyline sizes", "n_segments", n_segments);
    if (rc) return rc;
    if ((rc = sl_check_polylines("slice polyline sizes", n_polylines, n_segments))) return rc;
    if (!n_segments_out || !n_points_out) return nksr_set_error(NKSR_ERR_ARG, "slice polyline sizes: NULL arrays");
    if (n_segments > 0 && (!rep || !rank || !cyclic || !succ || !rep_dense || !polyline_of_dense || !segment_polyline_out || !closed_out))
        return nksr_set_error(NKSR_ERR_ARG, "slice polyline sizes: NULL arrays");
    MESH_LAUNCH(k_sl_poly_sizes, n_segments > 0 ? n_segments : 1, (hipStream_t)stream, rep, rank, cyclic, succ, n_segments, rep_dense, polyline_of_dense,
                n_polylines, segment_polyline_out, n_segments_out, n_points_out, closed_out);
    return NKSR_OK;
}

extern "C" int nksr_slice_polylines(const int32_t* segments, const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_segments,
                                    const int32_t* segment_polyline, const int32_t* polyline_rep, const int32_t* segment_offset,
                                    const int32_t* point_offset, int64_t n_polylines, const double* points, int64_t n_points, const double* normal,
                                    int32_t* polyline_points_out, uint64_t* term_key_out, double* length_term_out, double* area_term_out,
                                    void* stream) {
    int rc = sl_check_count("slice polylines", "n_segments", n_segments);
    if (rc) return rc;
    if ((rc = sl_check_count("slice polylines", "n_points", n_points))) return rc;
    if ((rc = sl_check_polylines("slice polylines", n_polylines, n_segments))) return rc;
    if (n_segments == 0) return NKSR_OK;
    if (!segments || !rank || !cyclic || !succ || !segment_polyline || !polyline_rep || !segment_offset || !point_offset || !points || !normal ||
        !polyline_points_out || !term_key_out || !length_term_out || !area_term_out)
        return nksr_set_error(NKSR_ERR_ARG, "slice polylines: NULL arrays");
    MESH_LAUNCH(k_sl_poly_fill, n_segments, (hipStream_t)stream, segments, rank, cyclic, succ, n_segments, segment_polyline, polyline_rep, segment_offset,
                point_offset, points, normal[0], normal[1], normal[2], polyline_points_out, term_key_out, length_term_out, area_term_out);
    return NKSR_OK;
}
