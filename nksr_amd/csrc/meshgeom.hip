// Triangle-mesh geometry (nksr_amd/mesh_geometry.py: MeshGeometry; layouts in include/nksr_hip.h):
//   k_geom_directed_keys  two (source << 32 | target, edge id) pairs per unique edge of the topology's table
//   k_geom_row_starts     row starts of a sorted key list by lower bound per vertex (adjacency rows, corner rows)
//   k_geom_unpack         neighbours, per-entry edge id and edge class;  k_geom_vertex_kind  interior / boundary / unreferenced
//   k_geom_corner_keys    (vertex, corner id) of every corner, invalid faces behind a sentinel
//   k_geom_faces          fp64 corner angles, cotangents, unit normal and area of every face
//   k_geom_edge_weights   cotangent weight of every unique edge: the opposite corners of ALL its faces, in sorted half-edge order
//   k_geom_vertex_gather  normal sum, barycentric area and angle sum over a vertex's corner row
//   k_geom_curvature      cotangent Laplacian over a vertex's adjacency row, signed mean curvature
//   k_geom_smooth_step    x_out = x_in + w (mean of the neighbours - x_in): the Laplacian / Taubin step
// Every kernel is one lane per item and gather-bound.  No floating-point atomic: every sum runs in the order of its sorted row, so
// every result repeats bit for bit.  Positions are read in the caller's precision (fp32 or fp64); everything computed is fp64.
#include "common.h"
#include "mesh_dev.h"

// (gm_vec3, gm_sub, gm_dot, gm_cross, gm_pos: mesh_dev.h)
__device__ __forceinline__ gm_vec3 gm_row(const double* x, int64_t i) { return {x[i * 3], x[i * 3 + 1], x[i * 3 + 2]}; }
__device__ __forceinline__ void gm_store(double* x, int64_t i, gm_vec3 p) { x[i * 3] = p.x; x[i * 3 + 1] = p.y; x[i * 3 + 2] = p.z; }

// ---- 1. directed adjacency -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_directed_keys(const int32_t* __restrict__ edges, int64_t ne, uint64_t* __restrict__ keys,
                                                                   uint32_t* __restrict__ ids) {
    const int64_t e = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (e >= ne) return;
    const uint64_t a = (uint64_t)(uint32_t)edges[e * 2], b = (uint64_t)(uint32_t)edges[e * 2 + 1];
    keys[e * 2] = (a << 32) | b;
    keys[e * 2 + 1] = (b << 32) | a;
    ids[e * 2] = (uint32_t)e;
    ids[e * 2 + 1] = (uint32_t)e;
}

// start[v] = the first sorted position whose key is >= v << shift, for v in [0, nv]: rows of equal (key >> shift), and at [nv] the
// position of the first key behind every vertex (the sentinels of the corner list, or n)
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_row_starts(const uint64_t* __restrict__ keys, int64_t n, int64_t nv, int shift,
                                                                uint32_t* __restrict__ start) {
    const int64_t v = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v > nv) return;
    const uint64_t target = (uint64_t)v << shift;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    start[v] = (uint32_t)lo;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_geom_unpack(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ eids, int64_t n,
                                                            const uint8_t* __restrict__ edge_class, int32_t* __restrict__ nbr,
                                                            int32_t* __restrict__ nbr_edge, uint8_t* __restrict__ nbr_class) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = eids[i];
    nbr[i] = (int32_t)(keys[i] & 0xFFFFFFFFull);
    nbr_edge[i] = (int32_t)e;
    nbr_class[i] = edge_class[e];
}

__global__ void __launch_bounds__(MESH_BLOCK) k_geom_vertex_kind(const uint32_t* __restrict__ start, const uint8_t* __restrict__ nbr_class,
                                                                 const uint8_t* __restrict__ vertex_ref, int64_t nv, uint8_t* __restrict__ kind) {
    const int64_t v = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= nv) return;
    int k = NKSR_GEOM_UNREFERENCED;
    if (vertex_ref[v]) {
        k = NKSR_GEOM_INTERIOR;
        for (int64_t i = start[v], end = start[v + 1]; i < end; ++i)
            if (nbr_class[i] == NKSR_TOPO_BOUNDARY) k = NKSR_GEOM_ON_BOUNDARY;
    }
    kind[v] = (uint8_t)k;
}

// ---- 2. vertex -> corner incidence -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_corner_keys(const void* faces, int is64, int64_t nf, int64_t nv,
                                                                 const uint8_t* __restrict__ face_valid, uint64_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ ids) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= nf) return;
    const bool ok = face_valid[j] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        keys[j * 3 + k] = ok ? (uint64_t)mesh_face_index(faces, is64, j * 3 + k) : (uint64_t)nv;     // nv: behind every vertex
        ids[j * 3 + k] = (uint32_t)(j * 3 + k);
    }
}

// ---- 3. per face -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_faces(const void* v, int v_f64, const void* faces, int is64, int64_t nf,
                                                           const uint8_t* __restrict__ face_valid, double* __restrict__ angle,
                                                           double* __restrict__ cot, double* __restrict__ normal, double* __restrict__ area) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= nf) return;
    if (!face_valid[j]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { angle[j * 3 + k] = 0.0; cot[j * 3 + k] = 0.0; normal[j * 3 + k] = 0.0; }
        area[j] = 0.0;
        return;
    }
    gm_vec3 p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = gm_pos(v, v_f64, mesh_face_index(faces, is64, j * 3 + k));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const gm_vec3 e1 = gm_sub(p[(k + 1) % 3], p[k]), e2 = gm_sub(p[(k + 2) % 3], p[k]);
        const gm_vec3 c = gm_cross(e1, e2);
        const double s = sqrt(gm_dot(c, c)), d = gm_dot(e1, e2);
        angle[j * 3 + k] = atan2(s, d);
        cot[j * 3 + k] = d / s;
    }
    const gm_vec3 n = gm_cross(gm_sub(p[1], p[0]), gm_sub(p[2], p[0]));
    const double len = sqrt(gm_dot(n, n));
    area[j] = 0.5 * len;
    normal[j * 3] = len > 0.0 ? n.x / len : 0.0;
    normal[j * 3 + 1] = len > 0.0 ? n.y / len : 0.0;
    normal[j * 3 + 2] = len > 0.0 ? n.z / len : 0.0;
}

// ---- 4. per edge -----------------------------------------------------------------------------------------------------------------
// half-edge h = 3 f + k runs corner k -> corner k + 1: the corner opposite is k + 2
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_edge_weights(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ edge_start,
                                                                  int64_t ne, const double* __restrict__ cot, double* __restrict__ weight) {
    const int64_t e = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (e >= ne) return;
    double w = 0.0;
    for (int64_t i = edge_start[e], end = edge_start[e + 1]; i < end; ++i) {
        const uint32_t h = ids[i];
        const uint32_t k = h % 3u;
        w += cot[(int64_t)(h - k) + (k + 2u) % 3u];
    }
    weight[e] = w;
}

// ---- 5. per vertex ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_vertex_gather(const uint32_t* __restrict__ corner_start, const uint32_t* __restrict__ corner_ids,
                                                                   int64_t nv, const double* __restrict__ angle, const double* __restrict__ face_normal,
                                                                   const double* __restrict__ face_area, int weighting, double* __restrict__ normal_out,
                                                                   double* __restrict__ area_out, double* __restrict__ angle_out) {
    const int64_t v = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= nv) return;
    gm_vec3 n = {0.0, 0.0, 0.0};
    double a_sum = 0.0, t_sum = 0.0;
    for (int64_t i = corner_start[v], end = corner_start[v + 1]; i < end; ++i) {
        const uint32_t c = corner_ids[i];
        const int64_t f = c / 3u;
        const double th = angle[c], a = face_area[f];
        const double w = weighting == NKSR_GEOM_WEIGHT_AREA ? a : th;
        n.x += w * face_normal[f * 3];
        n.y += w * face_normal[f * 3 + 1];
        n.z += w * face_normal[f * 3 + 2];
        a_sum += a;
        t_sum += th;
    }
    if (normal_out) {
        const double len = sqrt(gm_dot(n, n));
        const gm_vec3 u = {len > 0.0 ? n.x / len : 0.0, len > 0.0 ? n.y / len : 0.0, len > 0.0 ? n.z / len : 0.0};
        gm_store(normal_out, v, u);
    }
    if (area_out) area_out[v] = a_sum / 3.0;
    if (angle_out) angle_out[v] = t_sum;
}

// lap = (1 / 2A) sum_j w_ij (x_j - x_i);  H = |lap| / 2 * sgn(-lap . n);  NaN off the interior and where A = 0
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_curvature(const void* pos, int v_f64, int64_t nv, const uint32_t* __restrict__ start,
                                                               const int32_t* __restrict__ nbr, const int32_t* __restrict__ nbr_edge,
                                                               const double* __restrict__ edge_weight, const double* __restrict__ vertex_area,
                                                               const double* __restrict__ normal, const uint8_t* __restrict__ kind,
                                                               double* __restrict__ lap_out, double* __restrict__ h_out) {
    const int64_t v = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const gm_vec3 xi = gm_pos(pos, v_f64, v);
    gm_vec3 s = {0.0, 0.0, 0.0};
    for (int64_t i = start[v], end = start[v + 1]; i < end; ++i) {
        const gm_vec3 d = gm_sub(gm_pos(pos, v_f64, nbr[i]), xi);
        const double w = edge_weight[nbr_edge[i]];
        s.x += w * d.x;
        s.y += w * d.y;
        s.z += w * d.z;
    }
    const double a = vertex_area[v];
    const bool defined = kind[v] == NKSR_GEOM_INTERIOR && a > 0.0;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const gm_vec3 lap = {defined ? s.x / (2.0 * a) : nan, defined ? s.y / (2.0 * a) : nan, defined ? s.z / (2.0 * a) : nan};
    if (lap_out) gm_store(lap_out, v, lap);
    if (h_out) {
        const double along = -gm_dot(lap, gm_row(normal, v));
        const double sign = along > 0.0 ? 1.0 : (along < 0.0 ? -1.0 : 0.0);
        h_out[v] = defined ? 0.5 * sqrt(gm_dot(lap, lap)) * sign : nan;
    }
}

// ---- 6. the smoothing step -------------------------------------------------------------------------------------------------------
// A vertex stays (its row is copied) when it is unreferenced, flagged in `fixed`, or on a boundary edge under NKSR_GEOM_FIXED.  Under
// NKSR_GEOM_CURVE a boundary vertex averages the neighbours it reaches over boundary-class edges only.  Uniform weights over the row.
__global__ void __launch_bounds__(MESH_BLOCK) k_geom_smooth_step(const double* __restrict__ x_in, double* __restrict__ x_out, int64_t nv,
                                                                 const uint32_t* __restrict__ start, const int32_t* __restrict__ nbr,
                                                                 const uint8_t* __restrict__ nbr_class, const uint8_t* __restrict__ kind,
                                                                 const uint8_t* __restrict__ fixed, int boundary, double w) {
    const int64_t v = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const gm_vec3 xi = gm_row(x_in, v);
    const int k = kind[v];
    gm_vec3 out = xi;
    const bool stays = k == NKSR_GEOM_UNREFERENCED || (fixed && fixed[v]) || (k == NKSR_GEOM_ON_BOUNDARY && boundary == NKSR_GEOM_FIXED);
    if (!stays) {
        const bool curve = k == NKSR_GEOM_ON_BOUNDARY && boundary == NKSR_GEOM_CURVE;
        gm_vec3 s = {0.0, 0.0, 0.0};
        int64_t cnt = 0;
        for (int64_t i = start[v], end = start[v + 1]; i < end; ++i) {
            if (curve && nbr_class[i] != NKSR_TOPO_BOUNDARY) continue;
            const gm_vec3 xj = gm_row(x_in, nbr[i]);
            s.x += xj.x;
            s.y += xj.y;
            s.z += xj.z;
            ++cnt;
        }
        if (cnt > 0) {
            const double inv = 1.0 / (double)cnt;
            out.x = xi.x + w * (s.x * inv - xi.x);
            out.y = xi.y + w * (s.y * inv - xi.y);
            out.z = xi.z + w * (s.z * inv - xi.z);
        }
    }
    gm_store(x_out, v, out);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
// the unique edges of nf <= 2^30 faces: at most 3 * 2^30, and 2 E directed entries must fit the uint32 row starts
static int gm_check_edges(const char* who, int64_t nv, int64_t ne) {
    if (nv < 0 || ne < 0) return nksr_set_error(NKSR_ERR_ARG, "%s: negative size (nv=%lld, n_edges=%lld)", who, (long long)nv, (long long)ne);
    if (nv >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: nv=%lld, at most 2^31 - 1 vertices", who, (long long)nv);
    if (ne >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: n_edges=%lld, at most 2^31 - 1 edges", who, (long long)ne);
    return NKSR_OK;
}

extern "C" int nksr_geom_directed_keys(const int32_t* edges, int64_t n_edges, int64_t nv, uint64_t* keys_out, uint32_t* ids_out, void* stream) {
    int rc = gm_check_edges("geom directed keys", nv, n_edges);
    if (rc) return rc;
    if (n_edges == 0) return NKSR_OK;
    if (!edges || !keys_out || !ids_out) return nksr_set_error(NKSR_ERR_ARG, "geom directed keys: NULL arrays");
    MESH_LAUNCH(k_geom_directed_keys, n_edges, (hipStream_t)stream, edges, n_edges, keys_out, ids_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_adjacency(const uint64_t* keys_sorted, const uint32_t* edge_ids_sorted, int64_t n_edges, int64_t nv,
                                   const uint8_t* vertex_ref, const uint8_t* edge_class, uint32_t* start_out, int32_t* neighbour_out,
                                   int32_t* neighbour_edge_out, uint8_t* neighbour_class_out, uint8_t* vertex_kind_out, void* stream) {
    int rc = gm_check_edges("geom adjacency", nv, n_edges);
    if (rc) return rc;
    if (!start_out || (nv > 0 && (!vertex_ref || !vertex_kind_out)) ||
        (n_edges > 0 && (!keys_sorted || !edge_ids_sorted || !edge_class || !neighbour_out || !neighbour_edge_out || !neighbour_class_out)))
        return nksr_set_error(NKSR_ERR_ARG, "geom adjacency: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = 2 * n_edges;
    MESH_LAUNCH(k_geom_row_starts, nv + 1, st, keys_sorted, n, nv, 32, start_out);
    if (n > 0) MESH_LAUNCH(k_geom_unpack, n, st, keys_sorted, edge_ids_sorted, n, edge_class, neighbour_out, neighbour_edge_out, neighbour_class_out);
    if (nv > 0) MESH_LAUNCH(k_geom_vertex_kind, nv, st, start_out, neighbour_class_out, vertex_ref, nv, vertex_kind_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_corner_keys(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint8_t* face_valid, uint64_t* keys_out,
                                     uint32_t* ids_out, void* stream) {
    int rc = mesh_check_sizes("geom corner keys", nv, nf);
    if (rc) return rc;
    if (nf == 0) return NKSR_OK;
    if (!faces || !face_valid || !keys_out || !ids_out) return nksr_set_error(NKSR_ERR_ARG, "geom corner keys: NULL arrays");
    MESH_LAUNCH(k_geom_corner_keys, nf, (hipStream_t)stream, faces, faces_int64, nf, nv, face_valid, keys_out, ids_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_corner_rows(const uint64_t* keys_sorted, int64_t n_half, int64_t nv, uint32_t* start_out, void* stream) {
    if (n_half < 0 || n_half % 3 != 0)
        return nksr_set_error(NKSR_ERR_ARG, "geom corner rows: n_half=%lld is not three times a face count", (long long)n_half);
    int rc = mesh_check_sizes("geom corner rows", nv, n_half / 3);
    if (rc) return rc;
    if (!start_out || (n_half > 0 && !keys_sorted)) return nksr_set_error(NKSR_ERR_ARG, "geom corner rows: NULL arrays");
    MESH_LAUNCH(k_geom_row_starts, nv + 1, (hipStream_t)stream, keys_sorted, n_half, nv, 0, start_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_faces(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint8_t* face_valid,
                               double* angle_out, double* cot_out, double* normal_out, double* area_out, void* stream) {
    int rc = mesh_check_sizes("geom faces", nv, nf);
    if (rc) return rc;
    if (nf == 0) return NKSR_OK;
    if (!v || !faces || !face_valid || !angle_out || !cot_out || !normal_out || !area_out) return nksr_set_error(NKSR_ERR_ARG, "geom faces: NULL arrays");
    MESH_LAUNCH(k_geom_faces, nf, (hipStream_t)stream, v, v_float64, faces, faces_int64, nf, face_valid, angle_out, cot_out, normal_out, area_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_edge_weights(const uint32_t* ids_sorted, const uint32_t* edge_start, int64_t n_edges, int64_t nf, const double* cot,
                                      double* weight_out, void* stream) {
    int rc = mesh_check_sizes("geom edge weights", 0, nf);
    if (rc) return rc;
    if (n_edges < 0 || n_edges > 3 * nf)
        return nksr_set_error(NKSR_ERR_ARG, "geom edge weights: n_edges=%lld of %lld faces", (long long)n_edges, (long long)nf);
    if (n_edges == 0) return NKSR_OK;
    if (!ids_sorted || !edge_start || !cot || !weight_out) return nksr_set_error(NKSR_ERR_ARG, "geom edge weights: NULL arrays");
    MESH_LAUNCH(k_geom_edge_weights, n_edges, (hipStream_t)stream, ids_sorted, edge_start, n_edges, cot, weight_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_vertex_gather(const uint32_t* corner_start, const uint32_t* corner_ids, int64_t nv, int64_t nf, const double* angle,
                                       const double* face_normal, const double* face_area, int weighting, double* normal_out, double* area_out,
                                       double* angle_sum_out, void* stream) {
    int rc = mesh_check_sizes("geom vertex gather", nv, nf);
    if (rc) return rc;
    if (weighting != NKSR_GEOM_WEIGHT_ANGLE && weighting != NKSR_GEOM_WEIGHT_AREA)
        return nksr_set_error(NKSR_ERR_ARG, "geom vertex gather: weighting=%d is neither angle (0) nor area (1)", weighting);
    if (nv == 0) return NKSR_OK;
    if (!corner_start || (nf > 0 && (!corner_ids || !angle || !face_normal || !face_area)) || (!normal_out && !area_out && !angle_sum_out))
        return nksr_set_error(NKSR_ERR_ARG, "geom vertex gather: NULL arrays");
    MESH_LAUNCH(k_geom_vertex_gather, nv, (hipStream_t)stream, corner_start, corner_ids, nv, angle, face_normal, face_area, weighting, normal_out,
              area_out, angle_sum_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_curvature(const void* v, int v_float64, int64_t nv, const uint32_t* start, const int32_t* neighbour,
                                   const int32_t* neighbour_edge, int64_t n_edges, const double* edge_weight, const double* vertex_area,
                                   const double* vertex_normal, const uint8_t* vertex_kind, double* laplacian_out, double* mean_curvature_out,
                                   void* stream) {
    int rc = gm_check_edges("geom curvature", nv, n_edges);
    if (rc) return rc;
    if (nv == 0) return NKSR_OK;
    if (!v || !start || !vertex_area || !vertex_kind || (n_edges > 0 && (!neighbour || !neighbour_edge || !edge_weight)) ||
        (!laplacian_out && !mean_curvature_out) || (mean_curvature_out && !vertex_normal))
        return nksr_set_error(NKSR_ERR_ARG, "geom curvature: NULL arrays");
    MESH_LAUNCH(k_geom_curvature, nv, (hipStream_t)stream, v, v_float64, nv, start, neighbour, neighbour_edge, edge_weight, vertex_area, vertex_normal,
              vertex_kind, laplacian_out, mean_curvature_out);
    return NKSR_OK;
}

extern "C" int nksr_geom_smooth(double* x_a, double* x_b, int64_t nv, const uint32_t* start, const int32_t* neighbour, int64_t n_edges,
                                const uint8_t* neighbour_class, const uint8_t* vertex_kind, const uint8_t* fixed, int boundary, int64_t n_steps,
                                double w_even, double w_odd, void* stream) {
    int rc = gm_check_edges("geom smooth", nv, n_edges);
    if (rc) return rc;
    if (n_steps < 0) return nksr_set_error(NKSR_ERR_ARG, "geom smooth: negative size (n_steps=%lld)", (long long)n_steps);
    if (boundary != NKSR_GEOM_FIXED && boundary != NKSR_GEOM_CURVE && boundary != NKSR_GEOM_FREE)
        return nksr_set_error(NKSR_ERR_ARG, "geom smooth: boundary=%d is none of fixed (0), curve (1), free (2)", boundary);
    if (nv == 0 || n_steps == 0) return NKSR_OK;
    if (!x_a || !x_b || !start || !vertex_kind || (n_edges > 0 && (!neighbour || !neighbour_class)))
        return nksr_set_error(NKSR_ERR_ARG, "geom smooth: NULL arrays");
    if (x_a == x_b) return nksr_set_error(NKSR_ERR_ARG, "geom smooth: x_a and x_b are the same buffer");
    hipStream_t st = (hipStream_t)stream;
    for (int64_t s = 0; s < n_steps; ++s)           // no host synchronisation: the steps queue up behind one another
        MESH_LAUNCH(k_geom_smooth_step, nv, st, s & 1 ? x_b : x_a, s & 1 ? x_a : x_b, nv, start, neighbour, neighbour_class, vertex_kind, fixed,
                  boundary, s & 1 ? w_odd : w_even);
    return NKSR_OK;
}
