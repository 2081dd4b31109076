// Mesh simplification by quadric vertex clustering on a uniform grid (nksr_amd/mesh_simplify.py: MeshSimplifier; layouts in
// include/nksr_hip.h, definitions in DESIGN.md section 3.14):
//   k_simp_cell_keys        (cell key, vertex id) of every vertex: i = floor((double(x) - origin) / cell), an fp64 subtraction and an
//                           fp64 DIVISION (never a product with a reciprocal); unreferenced vertices behind the all-ones key
//   (the clusters are the runs of the sorted keys: nksr_run_counts_u64 / nksr_run_table_u64 of csrc/prims.hip)
//   k_simp_face_remap      cluster triple, valid / surviving flags and the two dedup sort keys of every face
//   k_simp_flag_duplicates  after the two stable sorts: a surviving face equal to its predecessor is a duplicate
//   k_simp_place            THE HOT KERNEL: one 16-lane group per cluster sums the quadric of the cluster's corner row, lane 0 solves
//   k_simp_cluster_means    fp64 mean of a [V, C] attribute over every cluster's vertex run
// The corner rows come from the geometry's entry points (nksr_geom_corner_keys / nksr_geom_corner_rows over the cluster triples), the
// final compaction from the topology's (nksr_topo_compact_*).  No floating-point atomic and no LDS: every sum runs in the fixed order
// of its sorted run and the 16 partial sums of a group meet in a fixed xor butterfly, so every result repeats bit for bit.
#include "common.h"
#include "mesh_dev.h"
#include "wave_dev.h"

#define SIMP_KEY_NONE 0xFFFFFFFFFFFFFFFFull
#define SIMP_INDEX_MASK ((1ull << 21) - 1ull)

// ---- 1. cell keys ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_simp_cell_keys(const void* v, int v_f64, int64_t nv, const int32_t* __restrict__ vertex_ref, double ox,
                                                               double oy, double oz, double cell, uint64_t* __restrict__ keys,
                                                               uint32_t* __restrict__ ids, int64_t* __restrict__ misfits) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool misfit = false;
    if (i < nv) {
        uint64_t key = SIMP_KEY_NONE;
        if (vertex_ref[i]) {
            const gm_vec3 p = gm_pos(v, v_f64, i);
            const double tx = floor((p.x - ox) / cell), ty = floor((p.y - oy) / cell), tz = floor((p.z - oz) / cell);
            const double lim = (double)NKSR_SIMP_MAX_INDEX;
            misfit = !(tx >= 0.0 && tx < lim && ty >= 0.0 && ty < lim && tz >= 0.0 && tz < lim);       // (a NaN is a misfit too)
            if (!misfit) key = ((uint64_t)tx << 42) | ((uint64_t)ty << 21) | (uint64_t)tz;
        }
        keys[i] = key;
        ids[i] = (uint32_t)i;
    }
    wave_count(misfit, misfits);
}

// ---- 2. faces --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_simp_face_remap(const void* faces, int is64, int64_t nf, int64_t nv, const int32_t* __restrict__ cluster_of,
                                                                void* cluster_faces, uint8_t* __restrict__ valid, uint8_t* __restrict__ survives,
                                                                uint64_t* __restrict__ key_ab, uint64_t* __restrict__ key_c, uint32_t* __restrict__ ids,
                                                                int64_t* __restrict__ counts) {
    const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool ok = false, collapsed = false;
    if (j < nf) {
        int64_t c[3];
        ok = mesh_valid_face(faces, is64, j, nv, c);
        int64_t g[3] = {0, 0, 0};                                    // an invalid face: a triple the compaction drops as well
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = cluster_of[c[k]];
            ok = g[0] >= 0 && g[1] >= 0 && g[2] >= 0;               // (always: a vertex of a valid face is referenced)
        }
        collapsed = ok && (g[0] == g[1] || g[1] == g[2] || g[0] == g[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (is64) ((int64_t*)cluster_faces)[j * 3 + k] = g[k];
            else ((int32_t*)cluster_faces)[j * 3 + k] = (int32_t)g[k];
        }
        const bool alive = ok && !collapsed;
        // a < b < c of a surviving face; (0, 0) | 0 elsewhere, which no surviving face has (its b is at least 1)
        const int64_t lo01 = g[0] < g[1] ? g[0] : g[1], hi01 = g[0] < g[1] ? g[1] : g[0];
        const int64_t lo = lo01 < g[2] ? lo01 : g[2], hi = hi01 > g[2] ? hi01 : g[2], mid = g[0] + g[1] + g[2] - lo - hi;
        valid[j] = ok ? 1 : 0;
        survives[j] = alive ? 1 : 0;
        key_ab[j] = alive ? ((uint64_t)lo << 32) | (uint64_t)mid : 0ull;
        key_c[j] = alive ? (uint64_t)hi : 0ull;
        ids[j] = (uint32_t)j;
    }
    wave_count(j < nf && !ok, counts);
    wave_count(collapsed, counts + 1);
}

__global__ void __launch_bounds__(MESH_BLOCK) k_simp_flag_duplicates(const uint32_t* __restrict__ order, int64_t nf, const uint64_t* __restrict__ key_ab,
                                                                     const uint64_t* __restrict__ key_c, const uint8_t* __restrict__ survives,
                                                                     uint8_t* __restrict__ keep, int64_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool dup = false;
    if (i < nf) {
        const int64_t p = order[i];
        if (p < nf) {
            const bool alive = survives[p] != 0;
            if (alive && i > 0) {
                const int64_t q = order[i - 1];
                dup = q < nf && survives[q] != 0 && key_ab[q] == key_ab[p] && key_c[q] == key_c[p];
            }
            keep[p] = alive && !dup ? 1 : 0;
        }
    }
    wave_count(dup, count);
}

// ---- 3. the hot kernel: cluster quadrics and placement ---------------------------------------------------------------------------
// centre of the cell of a key; the product and the sum are rounded one after the other, as the restatement rounds them
__device__ __forceinline__ gm_vec3 sm_centre(uint64_t key, double ox, double oy, double oz, double cell) {
#pragma clang fp contract(off)
    const double ix = (double)(key >> 42), iy = (double)((key >> 21) & SIMP_INDEX_MASK), iz = (double)(key & SIMP_INDEX_MASK);
    const double hx = (ix + 0.5) * cell, hy = (iy + 0.5) * cell, hz = (iz + 0.5) * cell;
    return {ox + hx, oy + hy, oz + hz};
}
__device__ __forceinline__ double sm_group_sum(double x) {          // over the 16 lanes of a group: the fixed butterfly 8, 4, 2, 1
    x += __shfl_xor(x, 8, NKSR_SIMP_GROUP);
    x += __shfl_xor(x, 4, NKSR_SIMP_GROUP);
    x += __shfl_xor(x, 2, NKSR_SIMP_GROUP);
    x += __shfl_xor(x, 1, NKSR_SIMP_GROUP);
    return x;
}
__device__ __forceinline__ double sm_clamp(double x, double h) { return x < -h ? -h : (x > h ? h : x); }

// Lane j of a group takes the corners j, j + 16, ... of the cluster's row: the face of the corner is read again (three indices, three
// positions), its normal and area recomputed, and a nn^T (6 distinct entries) and a d n (3) go into 9 fp64 accumulators.  A row of n
// corners costs ceil(n / 16) trips.  Lane 0 then sums the cluster's vertex run for the mean, solves the regularised 3 x 3 system by
// Cholesky, clamps to the cell and writes.  Every group of a wavefront runs the butterfly, whether its cluster exists or not.
__global__ void __launch_bounds__(MESH_BLOCK) k_simp_place(const void* v, int v_f64, int64_t nv, const void* faces, int is64, int64_t nf,
                                                           const uint32_t* __restrict__ corner_start, const uint32_t* __restrict__ corner_ids,
                                                           const uint32_t* __restrict__ cluster_start, const uint32_t* __restrict__ vertex_ids,
                                                           const uint64_t* __restrict__ cluster_key, int64_t nk, double ox, double oy, double oz,
                                                           double cell, double mu, int placement, double* __restrict__ out) {
    const int64_t g = ((int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x) / NKSR_SIMP_GROUP;
    const int lane = threadIdx.x & (NKSR_SIMP_GROUP - 1);
    const bool on = g < nk;
    const gm_vec3 centre = on ? sm_centre(cluster_key[g], ox, oy, oz, cell) : gm_vec3{0.0, 0.0, 0.0};
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (on && placement == NKSR_SIMP_QUADRIC) {
        for (int64_t i = (int64_t)corner_start[g] + lane, end = corner_start[g + 1]; i < end; i += NKSR_SIMP_GROUP) {
            const int64_t t = corner_ids[i] / 3u;
            int64_t c[3];
            if (t >= nf || !mesh_valid_face(faces, is64, t, nv, c)) continue;          // (never: the rows hold corners of valid faces)
            const gm_vec3 p0 = gm_pos(v, v_f64, c[0]), p1 = gm_pos(v, v_f64, c[1]), p2 = gm_pos(v, v_f64, c[2]);
            const gm_vec3 n = gm_cross(gm_sub(p1, p0), gm_sub(p2, p0));
            const double len = sqrt(gm_dot(n, n));
            if (!(len > 0.0)) continue;                             // a face without area adds nothing
            const gm_vec3 u = {n.x / len, n.y / len, n.z / len};
            const double a = 0.5 * len, d = -gm_dot(u, gm_sub(p0, centre));
            a00 += a * u.x * u.x;
            a01 += a * u.x * u.y;
            a02 += a * u.x * u.z;
            a11 += a * u.y * u.y;
            a12 += a * u.y * u.z;
            a22 += a * u.z * u.z;
            b0 += a * d * u.x;
            b1 += a * d * u.y;
            b2 += a * d * u.z;
        }
    }
    a00 = sm_group_sum(a00);
    a01 = sm_group_sum(a01);
    a02 = sm_group_sum(a02);
    a11 = sm_group_sum(a11);
    a12 = sm_group_sum(a12);
    a22 = sm_group_sum(a22);
    b0 = sm_group_sum(b0);
    b1 = sm_group_sum(b1);
    b2 = sm_group_sum(b2);
    if (!on || lane != 0) return;
    gm_vec3 s = {0.0, 0.0, 0.0};
    const int64_t v0 = cluster_start[g], v1 = cluster_start[g + 1];
    for (int64_t i = v0; i < v1; ++i) {                              // ascending vertex index: the sort was stable
        const int64_t vid = vertex_ids[i];
        if (vid >= nv) continue;
        const gm_vec3 r = gm_sub(gm_pos(v, v_f64, vid), centre);
        s.x += r.x;
        s.y += r.y;
        s.z += r.z;
    }
    const double cnt = (double)(v1 > v0 ? v1 - v0 : 1);
    const gm_vec3 mean = {s.x / cnt, s.y / cnt, s.z / cnt};
    gm_vec3 x = mean;
    const double tau = a00 + a11 + a22;
    if (placement == NKSR_SIMP_QUADRIC && tau > 0.0) {
        // (A + mu tau I) x = -b + mu tau mean: positive definite, condition number <= 1 + 1 / mu
        const double r = mu * tau;
        const double m00 = a00 + r, m11 = a11 + r, m22 = a22 + r;
        const double r0 = r * mean.x - b0, r1 = r * mean.y - b1, r2 = r * mean.z - b2;
        const double l00 = sqrt(m00), l10 = a01 / l00, l20 = a02 / l00;
        const double l11 = sqrt(m11 - l10 * l10), l21 = (a12 - l20 * l10) / l11;
        const double l22 = sqrt(m22 - l20 * l20 - l21 * l21);
        const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = (r2 - l20 * y0 - l21 * y1) / l22;
        x.z = y2 / l22;
        x.y = (y1 - l21 * x.z) / l11;
        x.x = (y0 - l10 * x.y - l20 * x.z) / l00;
    }
    const double h = 0.5 * cell;
    out[g * 3] = centre.x + sm_clamp(x.x, h);
    out[g * 3 + 1] = centre.y + sm_clamp(x.y, h);
    out[g * 3 + 2] = centre.z + sm_clamp(x.z, h);
}

// ---- 4. attribute means ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_simp_cluster_means(const void* attr, int attr_f64, int64_t nv, int64_t nc,
                                                                   const uint32_t* __restrict__ cluster_start, const uint32_t* __restrict__ vertex_ids,
                                                                   int64_t nk, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= nk * nc) return;
    const int64_t g = i / nc, ch = i - g * nc;
    const int64_t v0 = cluster_start[g], v1 = cluster_start[g + 1];
    double s = 0.0;
    for (int64_t k = v0; k < v1; ++k) {
        const int64_t vid = vertex_ids[k];
        if (vid >= nv) continue;
        s += attr_f64 ? ((const double*)attr)[vid * nc + ch] : (double)((const float*)attr)[vid * nc + ch];
    }
    out[i] = s / (double)(v1 > v0 ? v1 - v0 : 1);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
static int sm_check_clusters(const char* who, int64_t nk, int64_t nv) {
    if (nk < 0 || nk > nv) return nksr_set_error(NKSR_ERR_ARG, "%s: n_clusters=%lld of %lld vertices", who, (long long)nk, (long long)nv);
    return NKSR_OK;
}
static int sm_check_grid(const char* who, const double* origin, double cell) {
    if (!origin) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL origin", who);
    if (!(cell > 0.0) || cell * 0.5 == cell) return nksr_set_error(NKSR_ERR_ARG, "%s: cell_size=%g is not positive and finite", who, cell);
    for (int k = 0; k < 3; ++k)
        if (origin[k] - origin[k] != 0.0) return nksr_set_error(NKSR_ERR_ARG, "%s: non-finite origin", who);
    return NKSR_OK;
}

extern "C" int nksr_simp_cell_keys(const void* v, int v_float64, int64_t nv, const int32_t* vertex_ref, const double* origin, double cell_size,
                                   uint64_t* keys_out, uint32_t* ids_out, int64_t* misfits_out, void* stream) {
    int rc = mesh_check_sizes("simp cell keys", nv, 0);
    if (rc) return rc;
    if ((rc = sm_check_grid("simp cell keys", origin, cell_size))) return rc;
    if (!misfits_out || (nv > 0 && (!v || !vertex_ref || !keys_out || !ids_out))) return nksr_set_error(NKSR_ERR_ARG, "simp cell keys: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(misfits_out, 0, sizeof(int64_t), st));
    if (nv > 0) MESH_LAUNCH(k_simp_cell_keys, nv, st, v, v_float64, nv, vertex_ref, origin[0], origin[1], origin[2], cell_size, keys_out, ids_out, misfits_out);
    return NKSR_OK;
}

extern "C" int nksr_simp_face_remap(const void* faces, int faces_int64, int64_t nf, int64_t nv, const int32_t* cluster_of, void* cluster_faces_out,
                                    uint8_t* valid_out, uint8_t* survives_out, uint64_t* key_ab_out, uint64_t* key_c_out, uint32_t* ids_out,
                                    int64_t* counts_out, void* stream) {
    int rc = mesh_check_sizes("simp face remap", nv, nf);
    if (rc) return rc;
    if (!counts_out || (nf > 0 && (!faces || !cluster_faces_out || !valid_out || !survives_out || !key_ab_out || !key_c_out || !ids_out)) ||
        (nf > 0 && nv > 0 && !cluster_of))
        return nksr_set_error(NKSR_ERR_ARG, "simp face remap: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(counts_out, 0, 2 * sizeof(int64_t), st));
    if (nf > 0)
        MESH_LAUNCH(k_simp_face_remap, nf, st, faces, faces_int64, nf, nv, cluster_of, cluster_faces_out, valid_out, survives_out, key_ab_out, key_c_out,
                  ids_out, counts_out);
    return NKSR_OK;
}

extern "C" int nksr_simp_flag_duplicates(const uint32_t* order, int64_t nf, const uint64_t* key_ab, const uint64_t* key_c, const uint8_t* survives,
                                         uint8_t* keep_out, int64_t* count_out, void* stream) {
    int rc = mesh_check_sizes("simp flag duplicates", 0, nf);
    if (rc) return rc;
    if (!count_out || (nf > 0 && (!order || !key_ab || !key_c || !survives || !keep_out))) return nksr_set_error(NKSR_ERR_ARG, "simp flag duplicates: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    NKSR_CHECK_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), st));
    if (nf > 0) MESH_LAUNCH(k_simp_flag_duplicates, nf, st, order, nf, key_ab, key_c, survives, keep_out, count_out);
    return NKSR_OK;
}

extern "C" int nksr_simp_place(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint32_t* corner_start,
                               const uint32_t* corner_ids, const uint32_t* cluster_start, const uint32_t* vertex_ids_sorted, const uint64_t* cluster_key,
                               int64_t n_clusters, const double* origin, double cell_size, double regularisation, int placement,
                               double* representative_out, void* stream) {
    int rc = mesh_check_sizes("simp place", nv, nf);
    if (rc) return rc;
    if ((rc = sm_check_clusters("simp place", n_clusters, nv))) return rc;
    if ((rc = sm_check_grid("simp place", origin, cell_size))) return rc;
    if (placement != NKSR_SIMP_QUADRIC && placement != NKSR_SIMP_MEAN)
        return nksr_set_error(NKSR_ERR_ARG, "simp place: placement=%d is neither quadric (0) nor mean (1)", placement);
    if (!(regularisation > 0.0 && regularisation <= 1.0))
        return nksr_set_error(NKSR_ERR_ARG, "simp place: regularisation=%g outside (0, 1]", regularisation);
    if (n_clusters == 0) return NKSR_OK;
    if (!v || !cluster_start || !vertex_ids_sorted || !cluster_key || !representative_out ||
        (placement == NKSR_SIMP_QUADRIC && (!faces || !corner_start || !corner_ids)))
        return nksr_set_error(NKSR_ERR_ARG, "simp place: NULL arrays");
    MESH_LAUNCH(k_simp_place, n_clusters * NKSR_SIMP_GROUP, (hipStream_t)stream, v, v_float64, nv, faces, faces_int64, nf, corner_start, corner_ids,
              cluster_start, vertex_ids_sorted, cluster_key, n_clusters, origin[0], origin[1], origin[2], cell_size, regularisation, placement,
              representative_out);
    return NKSR_OK;
}

extern "C" int nksr_simp_cluster_means(const void* attr, int attr_float64, int64_t nv, int64_t channels, const uint32_t* cluster_start,
                                       const uint32_t* vertex_ids_sorted, int64_t n_clusters, double* mean_out, void* stream) {
    int rc = mesh_check_sizes("simp cluster means", nv, 0);
    if (rc) return rc;
    if ((rc = sm_check_clusters("simp cluster means", n_clusters, nv))) return rc;
    if (channels < 0 || channels > (1 << 16)) return nksr_set_error(NKSR_ERR_ARG, "simp cluster means: channels=%lld outside [0, 65536]", (long long)channels);
    if (n_clusters * channels >= (1ll << 38))                       // one lane per entry: the grid must fit 2^31 - 1 blocks
        return nksr_set_error(NKSR_ERR_ARG, "simp cluster means: %lld clusters x %lld channels >= 2^38 entries", (long long)n_clusters, (long long)channels);
    if (n_clusters == 0 || channels == 0) return NKSR_OK;
    if (!attr || !cluster_start || !vertex_ids_sorted || !mean_out) return nksr_set_error(NKSR_ERR_ARG, "simp cluster means: NULL arrays");
    MESH_LAUNCH(k_simp_cluster_means, n_clusters * channels, (hipStream_t)stream, attr, attr_float64, nv, channels, cluster_start, vertex_ids_sorted,
              n_clusters, mean_out);
    return NKSR_OK;
}
