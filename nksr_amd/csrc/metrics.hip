// Mesh metrics (nksr_amd/metrics.py, the reference's metrics.MeshEvaluator called at models/nksr_net.py:298-310):
//   k_face_areas     unit normal + fp64 area of every triangle (the CDF over the areas: nksr_inclusive_sum_f64, prims.hip)
//   k_mesh_sample    area-uniform surface samples, sample i a pure function of (seed, i) (Philox4x32-10, header nksr_hip.h)
//   k_nn_metrics     nksr_nn_metrics: exact 1-NN of every query (the k = 1 pyramid search of knn_topk_dev.h, the exhaustive
//                    knn_topk_all behind it) with the mesh-metric epilogue, per-workgroup partials [NKSR_METRIC_FIELDS]
//   k_metric_reduce  column sums of those partials, one workgroup in a fixed order
#include "common.h"
#include "mesh_dev.h"
#include "knn_topk_dev.h"

// the three corners of face j in fp64; false when an index lies outside [0, nv)
__device__ __forceinline__ bool face_corners(const float* __restrict__ v, int64_t nv, const void* faces, int is64, int64_t j, double p[3][3]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int64_t vi = mesh_face_index(faces, is64, j * 3 + c);
        if (vi < 0 || vi >= nv) { ok = false; vi = 0; }
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = (double)v[vi * 3 + a];
    }
    return ok;
}

__global__ void __launch_bounds__(256) k_face_areas(const float* __restrict__ v, int64_t nv, const void* faces, int is64, int64_t nf,
                                                    float* __restrict__ normal, double* __restrict__ area) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nf) return;
    double p[3][3];
    const bool ok = face_corners(v, nv, faces, is64, j, p);
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double len = ok ? sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) : 0.0;
    area[j] = 0.5 * len;
    const double inv = len > 0.0 ? 1.0 / len : 0.0;
    normal[j * 3] = (float)(cr[0] * inv);
    normal[j * 3 + 1] = (float)(cr[1] * inv);
    normal[j * 3 + 2] = (float)(cr[2] * inv);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds of two 32x32 -> 64-bit products,
// the key bumped by the Weyl constants between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    }
}

__global__ void __launch_bounds__(256) k_mesh_sample(const float* __restrict__ v, int64_t nv, const void* faces, int is64, int64_t nf,
                                                     const double* __restrict__ cdf, const float* __restrict__ fnormal, int64_t n,
                                                     uint64_t seed, float* __restrict__ xyz, float* __restrict__ normal,
                                                     int64_t* __restrict__ face) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), 0u, 0u};
    philox4x32_10(r, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u0 = (double)(((uint64_t)r[0] << 21) ^ ((uint64_t)r[1] >> 11)) * 0x1p-53;
    const double u1 = (double)r[2] * 0x1p-32, u2 = (double)r[3] * 0x1p-32;
    const double total = cdf[nf - 1];
    double t = u0 * total;
    if (!(t < total)) t = nextafter(total, 0.0);           // (u0 total may round up to total: the last positive step still holds t)
    int64_t lo = 0, hi = nf;                                // first j with cdf[j] > t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int64_t j = lo < nf ? lo : nf - 1;
    double p[3][3];
    face_corners(v, nv, faces, is64, j, p);
    const double s = sqrt(u1), w0 = 1.0 - s, w1 = s * (1.0 - u2), w2 = s * u2;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        xyz[i * 3 + a] = (float)(w0 * p[0][a] + w1 * p[1][a] + w2 * p[2][a]);
        normal[i * 3 + a] = fnormal[j * 3 + a];
    }
    face[i] = j;
}

// ---- exact 1-NN of every query with the mesh-metric epilogue (nksr_amd/metrics.py) ----------------------------------------------------
// Every query gets its nearest point.  The pyramid search (k = 1) answers the queries it can reach; a query it cannot -- farther from
// the cloud than max_ring rings of the top level, or with a cell index outside the biased 21-bit key range -- takes the box-pruned pass
// over ALL top-level cells instead: the cell of the nearest box first, then every cell whose box is not farther than the best
// candidate so far, each descended like any other.  The top level has a handful of cells (PointPyramid stops at <= 8).
// One thread per query: dist = |q - p_nn| (fp64 from the fp32 coordinates), dot = |n_q . n_nn| of the two normals scaled to unit length
// (a zero normal gives 0).  Per workgroup, fp64 sums of d, d^2, dot and the counts of d <= t for the five thresholds, reduced over the
// block in a fixed tree order: the partials (and nksr_metric_reduce over them) are bitwise reproducible.
__global__ void __launch_bounds__(NKSR_NN_BLOCK) k_nn_metrics(KnnPyramid Parg, const int64_t* __restrict__ top_keys, int n_top,
                                                              const float* __restrict__ tnrm, const float* __restrict__ query,
                                                              const float* __restrict__ qnrm, int64_t nq, int max_ring, float* __restrict__ dist,
                                                              float* __restrict__ dot, double* __restrict__ partials) {
    static_assert(NKSR_NN_BLOCK == KNN_PYR_BLOCK, "one LDS slot row per thread");
    __shared__ double s_red[NKSR_METRIC_FIELDS][NKSR_NN_BLOCK];
    int* node;
    unsigned char* cursor;
    const KnnPyramid& P = knn_pyramid_lds(Parg, node, cursor);
    const int64_t i = (int64_t)blockIdx.x * NKSR_NN_BLOCK + threadIdx.x;
    double acc[NKSR_METRIC_FIELDS];
#pragma unroll
    for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) acc[f] = 0.0;
    if (i < nq) {
        const float q[3] = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
        TopK<1> top;
        const float lim = (float)(NKSR_BIAS0 >> 1);           // cell indices well inside the biased key range
        const bool in_range = fabsf(q[0] * P.inv_cell) < lim && fabsf(q[1] * P.inv_cell) < lim && fabsf(q[2] * P.inv_cell) < lim;
        if (!in_range || !knn_topk_pyramid<1>(P, q, 1, max_ring, top, node, cursor))
            knn_topk_all<1>(P, top_keys, n_top, q, 1, top, node, cursor);
        const int j = top.idx[0];
        double d = __builtin_nan(""), dt = 0.0;
        if (j >= 0) {
            const double ex = (double)q[0] - (double)P.xyz[j * 3], ey = (double)q[1] - (double)P.xyz[j * 3 + 1],
                         ez = (double)q[2] - (double)P.xyz[j * 3 + 2];
            d = sqrt(ex * ex + ey * ey + ez * ez);
            if (tnrm && qnrm) {
                const double ax = qnrm[i * 3], ay = qnrm[i * 3 + 1], az = qnrm[i * 3 + 2];
                const double bx = tnrm[j * 3], by = tnrm[j * 3 + 1], bz = tnrm[j * 3 + 2];
                const double la = fmax(sqrt(ax * ax + ay * ay + az * az), 1e-30), lb = fmax(sqrt(bx * bx + by * by + bz * bz), 1e-30);
                dt = fabs(ax * bx + ay * by + az * bz) / (la * lb);
            }
        }
        if (dist) dist[i] = (float)d;
        if (dot) dot[i] = (float)dt;
        const double th[NKSR_METRIC_NTHRESH] = NKSR_METRIC_THRESHOLDS;
        acc[0] = d; acc[1] = d * d; acc[2] = dt;
#pragma unroll
        for (int t = 0; t < NKSR_METRIC_NTHRESH; ++t) acc[3 + t] = d <= th[t] ? 1.0 : 0.0;
    }
    if (!partials) return;
#pragma unroll
    for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) s_red[f][threadIdx.x] = acc[f];
    __syncthreads();
    for (int s = NKSR_NN_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) s_red[f][threadIdx.x] += s_red[f][threadIdx.x + s];
        __syncthreads();
    }
    if ((int)threadIdx.x < NKSR_METRIC_FIELDS) partials[(int64_t)blockIdx.x * NKSR_METRIC_FIELDS + threadIdx.x] = s_red[threadIdx.x][0];
}

#define METRIC_REDUCE_BLOCK 256
__global__ void __launch_bounds__(METRIC_REDUCE_BLOCK) k_metric_reduce(const double* __restrict__ partials, int64_t nrows, double* __restrict__ out) {
    __shared__ double s[NKSR_METRIC_FIELDS][METRIC_REDUCE_BLOCK];
    double acc[NKSR_METRIC_FIELDS];
#pragma unroll
    for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) acc[f] = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += METRIC_REDUCE_BLOCK)         // rows t, t + 256, ... in order
#pragma unroll
        for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) acc[f] += partials[r * NKSR_METRIC_FIELDS + f];
#pragma unroll
    for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) s[f][threadIdx.x] = acc[f];
    __syncthreads();
    for (int h = METRIC_REDUCE_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int f = 0; f < NKSR_METRIC_FIELDS; ++f) s[f][threadIdx.x] += s[f][threadIdx.x + h];
        __syncthreads();
    }
    if ((int)threadIdx.x < NKSR_METRIC_FIELDS) out[threadIdx.x] = s[threadIdx.x][0];
}

extern "C" int nksr_mesh_face_areas(const float* v, int64_t nv, const void* faces, int faces_int64, int64_t nf, float* normal_out,
                                    double* area_out, void* stream) {
    if (nv < 0 || nf < 0) return nksr_set_error(NKSR_ERR_ARG, "face areas: negative size (nv=%lld, nf=%lld)", (long long)nv, (long long)nf);
    if (nf == 0) return NKSR_OK;
    if (nv == 0) return nksr_set_error(NKSR_ERR_ARG, "face areas: %lld faces over zero vertices", (long long)nf);
    if (!v || !faces || !normal_out || !area_out) return nksr_set_error(NKSR_ERR_ARG, "face areas: NULL arrays");
    hipLaunchKernelGGL(k_face_areas, dim3(nksr_blocks(nf, 256)), dim3(256), 0, (hipStream_t)stream, v, nv, faces, faces_int64, nf, normal_out,
                       area_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_mesh_sample(const float* v, int64_t nv, const void* faces, int faces_int64, int64_t nf, const double* cdf,
                                const float* face_normal, int64_t n, uint64_t seed, float* xyz_out, float* normal_out, int64_t* face_out,
                                void* stream) {
    if (nv < 0 || nf < 0 || n < 0)
        return nksr_set_error(NKSR_ERR_ARG, "mesh sample: negative size (nv=%lld, nf=%lld, n=%lld)", (long long)nv, (long long)nf, (long long)n);
    if (n == 0) return NKSR_OK;
    if (nf == 0 || nv == 0) return nksr_set_error(NKSR_ERR_ARG, "mesh sample: n_points=%lld with zero faces or vertices", (long long)n);
    if (!v || !faces || !cdf || !face_normal || !xyz_out || !normal_out || !face_out) return nksr_set_error(NKSR_ERR_ARG, "mesh sample: NULL arrays");
    hipLaunchKernelGGL(k_mesh_sample, dim3(nksr_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, v, nv, faces, faces_int64, nf, cdf,
                       face_normal, n, seed, xyz_out, normal_out, face_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_nn_metrics(const nksr_knn_pyramid_t* pyramid, const int64_t* top_keys, int32_t n_top, const float* normal_sorted,
                               const float* query, const float* query_normal, int64_t nq, int max_ring, float* dist_out, float* dot_out,
                               double* partials_out, void* stream) {
    if (nq < 0 || n_top < 0) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: negative size (nq=%lld, n_top=%d)", (long long)nq, n_top);
    if (nq == 0) return NKSR_OK;
    if (!query || !top_keys || n_top < 1) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: NULL query / top-level keys or an empty target");
    if (!dist_out && !dot_out && !partials_out) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: no output (dist, dot and partials all NULL)");
    if (dot_out && (!normal_sorted || !query_normal)) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: dot output needs both normal arrays");
    if (max_ring < 1) return nksr_set_error(NKSR_ERR_ARG, "nn metrics: max_ring must be >= 1 (got %d)", max_ring);
    KnnPyramid P;
    if (int rc = make_pyramid(P, pyramid)) return rc;
    hipLaunchKernelGGL(k_nn_metrics, dim3(nksr_blocks(nq, NKSR_NN_BLOCK)), dim3(NKSR_NN_BLOCK), 0, (hipStream_t)stream, P, top_keys, (int)n_top,
                       normal_sorted, query, query_normal, nq, max_ring, dist_out, dot_out, partials_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_metric_reduce(const double* partials, int64_t nrows, double* out, void* stream) {
    if (nrows < 0) return nksr_set_error(NKSR_ERR_ARG, "metric reduce: negative size");
    if (!partials || !out) return nksr_set_error(NKSR_ERR_ARG, "metric reduce: NULL arrays");
    hipLaunchKernelGGL(k_metric_reduce, dim3(1), dim3(METRIC_REDUCE_BLOCK), 0, (hipStream_t)stream, partials, nrows, out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
