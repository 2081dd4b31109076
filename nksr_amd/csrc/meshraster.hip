// Mesh rasterisation along a coordinate axis (nksr_amd/mesh_raster.py: MeshRasterizer; layouts in include/nksr_hip.h):
//   k_rs_boxes          validity, candidate box on the grid and candidate count of every face; one lane per face
//   k_rs_test           the coverage predicate and the height of one (face, pixel of its box); one lane per candidate
//   k_rs_flag_counts    covering candidates per block of NKSR_RASTER_BLOCK
//   k_rs_compact        the covering candidates in candidate order: (pixel, face, height) hits
//   k_rs_pixel_start    the first layer of every pixel, from the run table of the sorted pixel keys
//   k_rs_reduce         one lane per run of a pixel: its layers in ascending face id, its height, face and count
//   k_rs_sample         vertex attributes at the hit of the pixel's face; one lane per (pixel, group of 4 channels)
//   k_rs_horn           Horn's 3 x 3 gradient and the hillshade; one lane per pixel
// Forward rasterisation: no rays, no tree.  No atomics anywhere: a candidate's id is the scan of the box sizes plus its position in
// the box, a hit's id the scan of the flags, a layer's position comes out of a stable sort, and every write has one writer, so every
// array repeats bit for bit.  A lane never loops over a box: a face costs what its box holds.
#include "common.h"
#include "mesh_dev.h"

// The predicate, the heights, the attributes and the gradient are stated operation by operation: products and
// sums round separately, so numpy gives the same bits.
#pragma clang fp contract(off)

static_assert(MESH_BLOCK == NKSR_RASTER_BLOCK, "the flag counts are per block of the candidate kernels");

#define RS_STAGE 512                // scanned candidate starts a block keeps in LDS (4 KiB)
#define RS_ATTR_GROUP 4             // channels per lane

// coordinate k of vertex i of an fp32 (widened exactly) or fp64 position array
__device__ __forceinline__ double rs_coord(const void* v, int v_f64, int64_t i, int k) {
    return v_f64 ? ((const double*)v)[i * 3 + k] : (double)((const float*)v)[i * 3 + k];
}

__device__ __forceinline__ bool rs_finite(double x) { return x - x == 0.0; }

// pixel centre: one rounded product and one rounded sum ((k + 0.5) is exact)
__device__ __forceinline__ double rs_centre(double origin, double pixel, int32_t k) { return origin + ((double)k + 0.5) * pixel; }

// ---- 1. boxes ----------------------------------------------------------------------------------------------------------------------
// The candidate box of a face along one axis: pixels floor((min - origin) / p) - 1 .. floor((max - origin) / p) + 1, clamped to
// [0, n).  Why the margin of one pixel is enough: a centre the predicate accepts lies in [min, max] of the face along the axis -- the
// differences x_a - X_i carry their exact signs, and a rounded edge function is never of the sign opposite to the exact one -- so its
// index is off the exact floor((x - origin) / p) of some x in [min, max] only by rounding.  X_i = origin + (i + 0.5) p is two rounded
// operations on values of at most M = max(|x|, |origin|) + p: off by at most 2 ulp(M) <= 2^-51 M.  (min - origin) / p is two rounded
// operations on a quotient of at most 2 M / p: off by at most 2^-50 M / p.  The host refuses p < 2^-40 M, so both errors are below
// 2^-10 of a pixel and the floor moves by at most one.  (The edge functions that round to zero are decided by the tie-break as if
// they were zero: a face thinner than an ulp that points at a far centre is the one case the argument leaves out.)
__device__ __forceinline__ bool rs_axis_box(double mn, double mx, double origin, double pixel, int64_t n, int32_t& lo, int32_t& hi) {
    const double dlo = floor((mn - origin) / pixel) - 1.0, dhi = floor((mx - origin) / pixel) + 1.0;
    if (!(dhi >= 0.0) || !(dlo <= (double)(n - 1))) return false;
    lo = dlo > 0.0 ? (int32_t)dlo : 0;
    hi = dhi < (double)(n - 1) ? (int32_t)dhi : (int32_t)(n - 1);
    return true;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_rs_boxes(const void* v, int v_f64, int64_t nv, const void* faces, int is64, int64_t nf, int ax,
                                                         int ay, double ox, double oy, double pixel, int64_t nx, int64_t ny,
                                                         uint8_t* __restrict__ face_valid, int32_t* __restrict__ box,
                                                         int64_t* __restrict__ count) {
    const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f == 0) count[nf] = 0;
    if (f >= nf) return;
    const int64_t a = mesh_face_index(faces, is64, f * 3), b = mesh_face_index(faces, is64, f * 3 + 1), c = mesh_face_index(faces, is64, f * 3 + 2);
    bool valid = a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv;
    int32_t i0 = 0, i1 = -1, j0 = 0, j1 = -1;
    int64_t n = 0;
    if (valid) {                    // (the vertices of a face with an index out of range are never read)
        const int az = 3 - ax - ay;
        const double xa = rs_coord(v, v_f64, a, ax), xb = rs_coord(v, v_f64, b, ax), xc = rs_coord(v, v_f64, c, ax);
        const double ya = rs_coord(v, v_f64, a, ay), yb = rs_coord(v, v_f64, b, ay), yc = rs_coord(v, v_f64, c, ay);
        const double za = rs_coord(v, v_f64, a, az), zb = rs_coord(v, v_f64, b, az), zc = rs_coord(v, v_f64, c, az);
        valid = rs_finite(xa) && rs_finite(xb) && rs_finite(xc) && rs_finite(ya) && rs_finite(yb) && rs_finite(yc) && rs_finite(za) &&
                rs_finite(zb) && rs_finite(zc);
        if (valid && nx > 0 && ny > 0 && rs_axis_box(fmin(xa, fmin(xb, xc)), fmax(xa, fmax(xb, xc)), ox, pixel, nx, i0, i1) &&
            rs_axis_box(fmin(ya, fmin(yb, yc)), fmax(ya, fmax(yb, yc)), oy, pixel, ny, j0, j1))
            n = (int64_t)(i1 - i0 + 1) * (int64_t)(j1 - j0 + 1);
    }
    face_valid[f] = valid ? 1 : 0;
    box[f * 4] = i0;
    box[f * 4 + 1] = i1;
    box[f * 4 + 2] = j0;
    box[f * 4 + 3] = j1;
    count[f] = n;
}

// ---- 2. the candidates -------------------------------------------------------------------------------------------------------------
// the last f in [lo, hi) with start[f] <= c (start[lo] <= c is the caller's business)
__device__ __forceinline__ int64_t rs_search(const int64_t* start, int64_t lo, int64_t hi, int64_t c) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (start[mid] <= c) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// The face of candidate c = blockIdx.x * MESH_BLOCK + threadIdx.x: the last one whose scanned start is <= c (a face without candidates
// shares its start with the next one and is never found).  Lanes 0 and 1 find the faces of the block's first and last candidate in
// the whole array; when the range between them fits, the block stages its starts in LDS and every lane searches there.  Called by
// every lane of the block (two barriers); -1 for a lane past the end.  cand_start[0] = 0 and c < n_cand = cand_start[nf] keep the
// result in [0, nf).
__device__ __forceinline__ int64_t rs_find_face(const int64_t* __restrict__ cand_start, int64_t nf, int64_t n_cand, int64_t c, int64_t* s_start,
                                                int64_t* s_range) {
    const int64_t c0 = (int64_t)blockIdx.x * MESH_BLOCK;
    if (threadIdx.x < 2) {
        const int64_t last = c0 + MESH_BLOCK < n_cand ? c0 + MESH_BLOCK - 1 : n_cand - 1;
        s_range[threadIdx.x] = rs_search(cand_start, 0, nf, threadIdx.x == 0 ? c0 : last);
    }
    __syncthreads();
    const int64_t f_lo = s_range[0], n = s_range[1] - f_lo + 1;
    const bool lds = n <= RS_STAGE;
    if (lds)
        for (int64_t k = threadIdx.x; k < n; k += MESH_BLOCK) s_start[k] = cand_start[f_lo + k];
    __syncthreads();
    if (c >= n_cand) return -1;
    return lds ? f_lo + rs_search(s_start, 0, n, c) : rs_search(cand_start, f_lo, f_lo + n, c);
}

// pixel (i, j) of candidate c of face f: its box row-major, j fastest, as the rasters are
__device__ __forceinline__ void rs_pixel(const int32_t* __restrict__ box, const int64_t* __restrict__ cand_start, int64_t f, int64_t c, int32_t& i,
                                         int32_t& j) {
    const int32_t i0 = box[f * 4], j0 = box[f * 4 + 2], w = box[f * 4 + 3] - j0 + 1;
    const int64_t local = c - cand_start[f];
    const int64_t row = local / w;
    i = i0 + (int32_t)row;
    j = j0 + (int32_t)(local - row * w);
}

// sign of the edge function e(P, Q) = Px Qy - Py Qx with the tie-break of mq_edge_sign (csrc/meshquery.hip) in fp64: antisymmetric
// bit for bit, s(Q, P) = -s(P, Q), so the two faces of an edge never both claim a centre on it and never both miss it
__device__ __forceinline__ int rs_edge_sign(double px, double py, double qx, double qy, double& e) {
    e = px * qy - py * qx;
    if (e > 0.0) return 1;
    if (e < 0.0) return -1;
    if (py != qy) return py > qy ? 1 : -1;
    if (qx != px) return qx > px ? 1 : -1;
    return 0;
}

struct rs_hit {
    double U, V, W, det;
    bool covered;
};

// the predicate of face (a, b, c) at the centre (X, Y)
__device__ __forceinline__ rs_hit rs_cover(const void* v, int v_f64, int64_t a, int64_t b, int64_t c, int ax, int ay, double X, double Y) {
    const double Ax = rs_coord(v, v_f64, a, ax) - X, Ay = rs_coord(v, v_f64, a, ay) - Y;
    const double Bx = rs_coord(v, v_f64, b, ax) - X, By = rs_coord(v, v_f64, b, ay) - Y;
    const double Cx = rs_coord(v, v_f64, c, ax) - X, Cy = rs_coord(v, v_f64, c, ay) - Y;
    rs_hit h;
    const int su = rs_edge_sign(Bx, By, Cx, Cy, h.U);
    const int sv = rs_edge_sign(Cx, Cy, Ax, Ay, h.V);
    const int sw = rs_edge_sign(Ax, Ay, Bx, By, h.W);
    h.det = (h.U + h.V) + h.W;
    h.covered = su != 0 && su == sv && su == sw && h.det != 0.0;
    return h;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_rs_test(const void* v, int v_f64, const void* faces, int is64, int64_t nf, int ax, int ay, double ox,
                                                        double oy, double pixel, const int32_t* __restrict__ box,
                                                        const int64_t* __restrict__ cand_start, int64_t n_cand, uint8_t* __restrict__ flag,
                                                        double* __restrict__ zf) {
    __shared__ int64_t s_start[RS_STAGE];
    __shared__ int64_t s_range[2];
    const int64_t c = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int64_t f = rs_find_face(cand_start, nf, n_cand, c, s_start, s_range);
    if (f < 0) return;
    int32_t i, j;
    rs_pixel(box, cand_start, f, c, i, j);
    const int64_t a = mesh_face_index(faces, is64, f * 3), b = mesh_face_index(faces, is64, f * 3 + 1), cc = mesh_face_index(faces, is64, f * 3 + 2);
    const rs_hit h = rs_cover(v, v_f64, a, b, cc, ax, ay, rs_centre(ox, pixel, i), rs_centre(oy, pixel, j));
    const int az = 3 - ax - ay;
    double z = 0.0;
    if (h.covered) z = ((h.U * rs_coord(v, v_f64, a, az) + h.V * rs_coord(v, v_f64, b, az)) + h.W * rs_coord(v, v_f64, cc, az)) / h.det;
    flag[c] = h.covered ? 1 : 0;
    zf[c] = z;
}

// ---- 3. compaction -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_rs_flag_counts(const uint8_t* __restrict__ flag, int64_t n_cand, int64_t n_blocks,
                                                               int64_t* __restrict__ counts) {
    const int64_t c = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int n = __syncthreads_count(c < n_cand && flag[c] != 0);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = n;
        if (blockIdx.x == 0) counts[n_blocks] = 0;
    }
}

// hit id = block_start[block] (the scan of the counts) + the covering candidates before this one in the block: candidate order, which
// is face order
__global__ void __launch_bounds__(MESH_BLOCK) k_rs_compact(const uint8_t* __restrict__ flag, const double* __restrict__ zf, const int32_t* __restrict__ box,
                                                           const int64_t* __restrict__ cand_start, int64_t nf, int64_t n_cand, int64_t ny,
                                                           const int64_t* __restrict__ block_start, uint64_t* __restrict__ hit_pixel,
                                                           int32_t* __restrict__ hit_face, double* __restrict__ hit_z) {
    __shared__ int64_t s_start[RS_STAGE];
    __shared__ int64_t s_range[2];
    __shared__ int32_t s_wave[MESH_BLOCK / 64];
    const int64_t c = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int64_t f = rs_find_face(cand_start, nf, n_cand, c, s_start, s_range);
    const bool hit = f >= 0 && flag[c] != 0;
    const uint64_t mask = __ballot(hit);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    if (!hit) return;
    int64_t id = block_start[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) id += s_wave[w];
    int32_t i, j;
    rs_pixel(box, cand_start, f, c, i, j);
    hit_pixel[id] = (uint64_t)((int64_t)i * ny + j);
    hit_face[id] = (int32_t)f;
    hit_z[id] = zf[c];
}

// ---- 4. layers and rasters ---------------------------------------------------------------------------------------------------------
// pixel_start[p] = the layers of the pixels before p: the start of the first run whose pixel is >= p, or all of them
__global__ void __launch_bounds__(MESH_BLOCK) k_rs_pixel_start(const uint64_t* __restrict__ run_keys, const int32_t* __restrict__ run_start, int64_t n_runs,
                                                               int64_t n_hits, int64_t n_pixels, int64_t* __restrict__ pixel_start) {
    const int64_t p = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (p > n_pixels) return;
    int64_t lo = 0, hi = n_runs;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (run_keys[mid] < (uint64_t)p) lo = mid + 1;
        else hi = mid;
    }
    pixel_start[p] = lo < n_runs ? (int64_t)(uint32_t)run_start[lo] : n_hits;
}

// One lane per run = per covered pixel.  The run is in ascending face id (the hits are, and the sort is stable), so the first layer
// that attains the best height is the lowest face id among them: only a strictly better height replaces it.
__global__ void __launch_bounds__(MESH_BLOCK) k_rs_reduce(const uint64_t* __restrict__ run_keys, const int32_t* __restrict__ run_start, int64_t n_runs,
                                                          const int32_t* __restrict__ order, const int32_t* __restrict__ hit_face,
                                                          const double* __restrict__ hit_z, int bottom, int32_t* __restrict__ layer_face,
                                                          double* __restrict__ layer_height, double* __restrict__ height,
                                                          int32_t* __restrict__ face, int32_t* __restrict__ count) {
    const int64_t r = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (r >= n_runs) return;
    const int64_t s = (uint32_t)run_start[r], e = (uint32_t)run_start[r + 1];
    double best = 0.0;
    int32_t best_face = -1;
    for (int64_t k = s; k < e; ++k) {
        const int64_t h = order[k];
        const double z = hit_z[h];
        const int32_t f = hit_face[h];
        layer_face[k] = f;
        layer_height[k] = z;
        if (k == s || (bottom ? z < best : z > best)) {
            best = z;
            best_face = f;
        }
    }
    const int64_t p = (int64_t)run_keys[r];
    height[p] = best;
    face[p] = best_face;
    count[p] = (int32_t)(e - s);
}

// ---- 5. derived rasters ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_BLOCK) k_rs_sample(const void* v, int v_f64, int64_t nv, const void* faces, int is64, int64_t nf, int ax, int ay,
                                                          double ox, double oy, double pixel, int64_t ny, int64_t n_pixels,
                                                          const int32_t* __restrict__ face_map, const void* attr, int attr_f64, int64_t channels,
                                                          int64_t groups, double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (q >= n_pixels * groups) return;
    const int64_t p = q / groups, c0 = (q - p * groups) * RS_ATTR_GROUP;
    const int64_t c1 = c0 + RS_ATTR_GROUP < channels ? c0 + RS_ATTR_GROUP : channels;
    const int64_t f = face_map[p];
    int64_t a = -1, b = -1, c = -1;
    if (f >= 0 && f < nf) {
        a = mesh_face_index(faces, is64, f * 3);
        b = mesh_face_index(faces, is64, f * 3 + 1);
        c = mesh_face_index(faces, is64, f * 3 + 2);
    }
    if (!(a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv)) {      // an empty pixel (or a map that is not this mesh's)
        for (int64_t k = c0; k < c1; ++k) out[p * channels + k] = __builtin_nan("");
        return;
    }
    const int64_t i = p / ny;
    const rs_hit h = rs_cover(v, v_f64, a, b, c, ax, ay, rs_centre(ox, pixel, (int32_t)i), rs_centre(oy, pixel, (int32_t)(p - i * ny)));
    for (int64_t k = c0; k < c1; ++k) {
        const double ta = attr_f64 ? ((const double*)attr)[a * channels + k] : (double)((const float*)attr)[a * channels + k];
        const double tb = attr_f64 ? ((const double*)attr)[b * channels + k] : (double)((const float*)attr)[b * channels + k];
        const double tc = attr_f64 ? ((const double*)attr)[c * channels + k] : (double)((const float*)attr)[c * channels + k];
        out[p * channels + k] = ((h.U * ta + h.V * tb) + h.W * tc) / h.det;
    }
}

// Horn's differences over the 3 x 3 neighbourhood and the shade of the unit sun vector (sx, sy, sz); NaN on the rim and wherever one of
// the nine heights is missing
__global__ void __launch_bounds__(MESH_BLOCK) k_rs_horn(const double* __restrict__ h, int64_t nx, int64_t ny, double pixel, double sx, double sy, double sz,
                                                        double* __restrict__ gx, double* __restrict__ gy, double* __restrict__ shade) {
    const int64_t p = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (p >= nx * ny) return;
    const int64_t i = p / ny, j = p - i * ny;
    double x = __builtin_nan(""), y = x, s = x;
    if (i > 0 && i < nx - 1 && j > 0 && j < ny - 1) {
        const double a = h[p - ny - 1], b = h[p - ny], c = h[p - ny + 1];         // row i - 1: j - 1, j, j + 1
        const double d = h[p - 1], m = h[p], e = h[p + 1];
        const double f = h[p + ny - 1], g = h[p + ny], k = h[p + ny + 1];         // row i + 1
        if (rs_finite(a) && rs_finite(b) && rs_finite(c) && rs_finite(d) && rs_finite(m) && rs_finite(e) && rs_finite(f) && rs_finite(g) &&
            rs_finite(k)) {
            const double scale = 8.0 * pixel;
            x = (((f + 2.0 * g) + k) - ((a + 2.0 * b) + c)) / scale;
            y = (((c + 2.0 * e) + k) - ((a + 2.0 * d) + f)) / scale;
            const double t = (sz - (sx * x + sy * y)) / sqrt((1.0 + x * x) + y * y);
            s = t > 0.0 ? t : 0.0;
        }
    }
    gx[p] = x;
    gy[p] = y;
    shade[p] = s;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
static int rs_check_count(const char* who, const char* what, int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: %s=%lld outside [0, 2^31)", who, what, (long long)n);
    return NKSR_OK;
}

static int rs_check_grid(const char* who, int ax, int ay, double ox, double oy, double pixel, int64_t nx, int64_t ny) {
    if (ax < 0 || ax > 2 || ay < 0 || ay > 2 || ax == ay) return nksr_set_error(NKSR_ERR_ARG, "%s: axes (%d, %d), expected two different of 0, 1, 2", who, ax, ay);
    if (!(pixel > 0.0) || pixel - pixel != 0.0 || ox - ox != 0.0 || oy - oy != 0.0)
        return nksr_set_error(NKSR_ERR_ARG, "%s: expected a positive finite pixel size and a finite origin", who);
    if (nx < 0 || ny < 0 || (ny > 0 && nx > ((1ll << 31) - 1) / ny))
        return nksr_set_error(NKSR_ERR_ARG, "%s: a grid of %lld x %lld pixels, nx ny outside [0, 2^31)", who, (long long)nx, (long long)ny);
    return NKSR_OK;
}

extern "C" int nksr_raster_boxes(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, int axis_x, int axis_y,
                                 double origin_x, double origin_y, double pixel_size, int64_t nx, int64_t ny, uint8_t* face_valid_out, int32_t* box_out,
                                 int64_t* count_out, void* stream) {
    int rc = mesh_check_sizes("raster boxes", nv, nf);
    if (rc) return rc;
    if ((rc = rs_check_grid("raster boxes", axis_x, axis_y, origin_x, origin_y, pixel_size, nx, ny))) return rc;
    if (!count_out || (nf > 0 && (!faces || !face_valid_out || !box_out)) || (nf > 0 && nv > 0 && !v))
        return nksr_set_error(NKSR_ERR_ARG, "raster boxes: NULL arrays");
    MESH_LAUNCH(k_rs_boxes, nf > 0 ? nf : 1, (hipStream_t)stream, v, v_float64, nv, faces, faces_int64, nf, axis_x, axis_y, origin_x, origin_y, pixel_size,
                nx, ny, face_valid_out, box_out, count_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_test(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, int axis_x, int axis_y,
                                double origin_x, double origin_y, double pixel_size, int64_t nx, int64_t ny, const int32_t* box,
                                const int64_t* cand_start, int64_t n_candidates, uint8_t* flag_out, double* height_out, void* stream) {
    int rc = mesh_check_sizes("raster test", nv, nf);
    if (rc) return rc;
    if ((rc = rs_check_grid("raster test", axis_x, axis_y, origin_x, origin_y, pixel_size, nx, ny))) return rc;
    if ((rc = rs_check_count("raster test", "n_candidates", n_candidates))) return rc;
    if (n_candidates == 0) return NKSR_OK;
    if (nf == 0 || nv == 0) return nksr_set_error(NKSR_ERR_ARG, "raster test: %lld candidates without faces or vertices", (long long)n_candidates);
    if (!v || !faces || !box || !cand_start || !flag_out || !height_out) return nksr_set_error(NKSR_ERR_ARG, "raster test: NULL arrays");
    MESH_LAUNCH(k_rs_test, n_candidates, (hipStream_t)stream, v, v_float64, faces, faces_int64, nf, axis_x, axis_y, origin_x, origin_y, pixel_size, box,
                cand_start, n_candidates, flag_out, height_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_flag_counts(const uint8_t* flag, int64_t n_candidates, int64_t* counts_out, void* stream) {
    int rc = rs_check_count("raster flag counts", "n_candidates", n_candidates);
    if (rc) return rc;
    if (!counts_out || (n_candidates > 0 && !flag)) return nksr_set_error(NKSR_ERR_ARG, "raster flag counts: NULL arrays");
    if (n_candidates == 0) { NKSR_CHECK_HIP(hipMemsetAsync(counts_out, 0, sizeof(int64_t), (hipStream_t)stream)); return NKSR_OK; }
    MESH_LAUNCH(k_rs_flag_counts, n_candidates, (hipStream_t)stream, flag, n_candidates, (int64_t)nksr_blocks(n_candidates, MESH_BLOCK), counts_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_compact(const uint8_t* flag, const double* height, const int32_t* box, const int64_t* cand_start, int64_t nf,
                                   int64_t n_candidates, int64_t nx, int64_t ny, const int64_t* block_start, int64_t n_hits, uint64_t* hit_pixel_out,
                                   int32_t* hit_face_out, double* hit_height_out, void* stream) {
    int rc = mesh_check_sizes("raster compact", 0, nf);
    if (rc) return rc;
    if ((rc = rs_check_count("raster compact", "n_candidates", n_candidates))) return rc;
    if ((rc = rs_check_grid("raster compact", 0, 1, 0.0, 0.0, 1.0, nx, ny))) return rc;
    if (n_hits < 0 || n_hits > n_candidates)
        return nksr_set_error(NKSR_ERR_ARG, "raster compact: %lld hits of %lld candidates", (long long)n_hits, (long long)n_candidates);
    if (n_hits == 0) return NKSR_OK;
    if (nf == 0) return nksr_set_error(NKSR_ERR_ARG, "raster compact: %lld hits without faces", (long long)n_hits);
    if (!flag || !height || !box || !cand_start || !block_start || !hit_pixel_out || !hit_face_out || !hit_height_out)
        return nksr_set_error(NKSR_ERR_ARG, "raster compact: NULL arrays");
    MESH_LAUNCH(k_rs_compact, n_candidates, (hipStream_t)stream, flag, height, box, cand_start, nf, n_candidates, ny, block_start, hit_pixel_out,
                hit_face_out, hit_height_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_pixel_start(const uint64_t* run_keys, const int32_t* run_start, int64_t n_runs, int64_t n_hits, int64_t n_pixels,
                                       int64_t* pixel_start_out, void* stream) {
    int rc = rs_check_count("raster pixel start", "n_hits", n_hits);
    if (rc) return rc;
    if ((rc = rs_check_count("raster pixel start", "n_pixels", n_pixels))) return rc;
    if (n_runs < 0 || n_runs > n_hits || n_runs > n_pixels)
        return nksr_set_error(NKSR_ERR_ARG, "raster pixel start: %lld runs of %lld hits on %lld pixels", (long long)n_runs, (long long)n_hits,
                              (long long)n_pixels);
    if (!pixel_start_out || (n_runs > 0 && (!run_keys || !run_start))) return nksr_set_error(NKSR_ERR_ARG, "raster pixel start: NULL arrays");
    MESH_LAUNCH(k_rs_pixel_start, n_pixels + 1, (hipStream_t)stream, run_keys, run_start, n_runs, n_hits, n_pixels, pixel_start_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_reduce(const uint64_t* run_keys, const int32_t* run_start, int64_t n_runs, const int32_t* order, const int32_t* hit_face,
                                  const double* hit_height, int64_t n_hits, int bottom, int64_t n_pixels, int32_t* layer_face_out,
                                  double* layer_height_out, double* height_out, int32_t* face_out, int32_t* count_out, void* stream) {
    int rc = rs_check_count("raster reduce", "n_hits", n_hits);
    if (rc) return rc;
    if ((rc = rs_check_count("raster reduce", "n_pixels", n_pixels))) return rc;
    if (n_runs < 0 || n_runs > n_hits || n_runs > n_pixels)
        return nksr_set_error(NKSR_ERR_ARG, "raster reduce: %lld runs of %lld hits on %lld pixels", (long long)n_runs, (long long)n_hits, (long long)n_pixels);
    if (n_runs == 0) return NKSR_OK;
    if (!run_keys || !run_start || !order || !hit_face || !hit_height || !layer_face_out || !layer_height_out || !height_out || !face_out || !count_out)
        return nksr_set_error(NKSR_ERR_ARG, "raster reduce: NULL arrays");
    MESH_LAUNCH(k_rs_reduce, n_runs, (hipStream_t)stream, run_keys, run_start, n_runs, order, hit_face, hit_height, bottom, layer_face_out,
                layer_height_out, height_out, face_out, count_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_sample(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, int axis_x, int axis_y,
                                  double origin_x, double origin_y, double pixel_size, int64_t nx, int64_t ny, const int32_t* face_map, const void* attr,
                                  int attr_float64, int64_t channels, double* attr_out, void* stream) {
    int rc = mesh_check_sizes("raster sample", nv, nf);
    if (rc) return rc;
    if ((rc = rs_check_grid("raster sample", axis_x, axis_y, origin_x, origin_y, pixel_size, nx, ny))) return rc;
    if ((rc = rs_check_count("raster sample", "channels", channels))) return rc;
    const int64_t n_pixels = nx * ny;
    if (n_pixels == 0 || channels == 0) return NKSR_OK;
    const int64_t groups = (channels + RS_ATTR_GROUP - 1) / RS_ATTR_GROUP;
    if (groups > (1ll << 40) / n_pixels) return nksr_set_error(NKSR_ERR_ARG, "raster sample: %lld pixels of %lld channels", (long long)n_pixels, (long long)channels);
    if (!face_map || !attr_out || (nf > 0 && nv > 0 && (!v || !faces || !attr))) return nksr_set_error(NKSR_ERR_ARG, "raster sample: NULL arrays");
    MESH_LAUNCH(k_rs_sample, n_pixels * groups, (hipStream_t)stream, v, v_float64, nv, faces, faces_int64, nf, axis_x, axis_y, origin_x, origin_y, pixel_size,
                ny, n_pixels, face_map, attr, attr_float64, channels, groups, attr_out);
    return NKSR_OK;
}

extern "C" int nksr_raster_horn(const double* height, int64_t nx, int64_t ny, double pixel_size, const double* sun, double* gx_out, double* gy_out,
                                double* shade_out, void* stream) {
    int rc = rs_check_grid("raster horn", 0, 1, 0.0, 0.0, pixel_size, nx, ny);
    if (rc) return rc;
    if (!sun) return nksr_set_error(NKSR_ERR_ARG, "raster horn: NULL arrays");
    if (nx * ny == 0) return NKSR_OK;
    if (!height || !gx_out || !gy_out || !shade_out) return nksr_set_error(NKSR_ERR_ARG, "raster horn: NULL arrays");
    MESH_LAUNCH(k_rs_horn, nx * ny, (hipStream_t)stream, height, nx, ny, pixel_size, sun[0], sun[1], sun[2], gx_out, gy_out, shade_out);
    return NKSR_OK;
}
