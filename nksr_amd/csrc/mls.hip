// Moving-least-squares projection over a Morton-sorted cloud (nksr_amd/mls.py: cloud.mls_project, cloud.smooth_mls; the grid:
// nksr_amd/neighbours.py PointGrid with cell >= radius, as nksr_radius_count takes it).
//
//      k_mls_project<ORDER>   nksr_mls_project: one lane per query, queries in Morton order where they are the cloud itself.
//
// The definition (tests/mls_ref.py restates it in numpy).  h = the fp32 radius, s = sigma, q = the query.
//      neighbours   the points p with knn_d2(p - q) <= h * h in fp32, inclusive: the predicate and the count of k_radius_count
//      weights      w = exp(-|d|^2 / s^2) in fp64, d = p - q in fp64
//      plane        W = sum w, m = sum w d / W, C = sum w d d^T - W m m^T (about q, shifted: |d| <= h); eigenvalues l0 <= l1 <= l2 of C
//                   by cyclic Jacobi (eig3_dev.h), n = the eigenvector of l0, o = (m . n) n = the foot of q on the plane, relative to q
//      sign of n    with input normals n_i: flipped when (sum w n_i) . n < 0; without: the component of n with the largest magnitude is
//                   positive (ties: the lowest axis)
//      order 1      x' = q + o, the normal is n, the curvatures are NaN, variation = l0 / (l0 + l1 + l2)
//      order 2      frame (u, v, n) from the other two eigenvectors; a neighbour's r = d - o has x = r . u / h, y = r . v / h, z = r . n / h;
//                   z ~ a0 + a1 x + a2 y + a3 x^2 + a4 x y + a5 y^2 by the weighted 6 x 6 normal equations, Cholesky in fp64;
//                   x' = q + o + a0 h n, normal = (n - a1 u - a2 v) scaled to unit length; with fx = a1, fy = a2, fxx = 2 a3 / h, fxy = a4 / h,
//                   fyy = 2 a5 / h: K = (fxx fyy - fxy^2) / (1 + fx^2 + fy^2)^2,
//                   H = -((1 + fy^2) fxx - 2 fx fy fxy + (1 + fx^2) fyy) / (2 (1 + fx^2 + fy^2)^(3/2)): positive on a sphere with outward
//                   normals (MeshGeometry.mean_curvature's convention)
//      order_used   0: fewer than min_neighbors neighbours, W not positive, or l1 <= max(1e-12 l2, 1e-14 W h^2) (collinear / coincident
//                   neighbours; the second term is the rounding of the shifted sums, which leaves eigenvalues of that size where the
//                   exact ones are zero): the point comes back as it is, curvatures and variation are NaN, the normal is the point's
//                   input normal (self-queries with normals) or NaN; 1: the plane -- asked for, or order 2 with a Cholesky pivot
//                   <= 1e-12 x the largest diagonal entry of the normal equations; 2: the quadric
// Two walks over the 27 cells: the 10 moment sums and the 3 normal sums, then the 21 + 6 sums of the normal equations.  Every sum is fp64
// in the fixed order of the walk (knn_cells27, the points of a cell ascending), no atomics: the same call gives the same bits, and a
// query's row does not depend on the other queries of the launch.  Every loop over matrix entries is unrolled, so the accumulators live
// in registers (no scratch: hipcc -Rpass-analysis=kernel-resource-usage).
#include "common.h"
#include "eig3_dev.h"
#include "knn_dev.h"

#define MLS_RANK_TOL 1e-12
#define MLS_ROUNDING_FLOOR 1e-14          // x W h^2: below it an eigenvalue of the shifted covariance is rounding

__device__ __forceinline__ double mls_pick(int j, double x0, double x1, double x2) { return j == 0 ? x0 : (j == 1 ? x1 : x2); }

template <int ORDER>
__global__ void __launch_bounds__(128) k_mls_project(KnnGrid g, const float* __restrict__ nrm, const float* __restrict__ query, int64_t nq,
                                                     float r2, double h, double inv_s2, int min_nb, double* __restrict__ pos_out,
                                                     double* __restrict__ nrm_out, double* __restrict__ mean_out, double* __restrict__ gauss_out,
                                                     double* __restrict__ var_out, int32_t* __restrict__ count_out, int8_t* __restrict__ used_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float* qp = query ? query + i * 3 : g.xyz + i * 3;
    const float q[3] = {qp[0], qp[1], qp[2]};
    const double q0 = (double)q[0], q1 = (double)q[1], q2 = (double)q[2];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int c[3];
    cell_of(g, q, c);

    // ---- first walk: count, W, sum w d, sum w d d^T, sum w n_i ------------------------------------------------------------------
    int n = 0;
    double W = 0, sx = 0, sy = 0, sz = 0, cxx = 0, cxy = 0, cxz = 0, cyy = 0, cyz = 0, czz = 0, wnx = 0, wny = 0, wnz = 0;
    knn_cells27(g, c, [&](int ci) {
        knn_scan4(g.xyz, g.start[ci], g.end[ci], q, [&](int kk, float d2f) {
            if (!(d2f <= r2)) return;
            const double dx = (double)g.xyz[(int64_t)kk * 3] - q0, dy = (double)g.xyz[(int64_t)kk * 3 + 1] - q1,
                         dz = (double)g.xyz[(int64_t)kk * 3 + 2] - q2;
            const double w = exp(-((dx * dx + dy * dy) + dz * dz) * inv_s2);
            const double wx = w * dx, wy = w * dy, wz = w * dz;
            ++n;
            W += w;
            sx += wx; sy += wy; sz += wz;
            cxx += wx * dx; cxy += wx * dy; cxz += wx * dz;
            cyy += wy * dy; cyz += wy * dz; czz += wz * dz;
            if (nrm) {
                wnx += w * (double)nrm[(int64_t)kk * 3]; wny += w * (double)nrm[(int64_t)kk * 3 + 1]; wnz += w * (double)nrm[(int64_t)kk * 3 + 2];
            }
        });
        return true;
    });
    count_out[i] = n;

    // what an order_used = 0 row holds; overwritten below by what the fits give
    int used = 0;
    double px = q0, py = q1, pz = q2, onx = nan, ony = nan, onz = nan, Hc = nan, Kc = nan, var = nan;
    if (nrm && !query) { onx = (double)nrm[i * 3]; ony = (double)nrm[i * 3 + 1]; onz = (double)nrm[i * 3 + 2]; }

    if (n >= min_nb && W > 0.0) {
        const double mx = sx / W, my = sy / W, mz = sz / W;
        double a[3][3], ev[3][3];
        a[0][0] = cxx - sx * mx; a[0][1] = cxy - sx * my; a[0][2] = cxz - sx * mz;
        a[1][1] = cyy - sy * my; a[1][2] = cyz - sy * mz; a[2][2] = czz - sz * mz;
        a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[2][1] = a[1][2];
        jacobi_eig3(a, ev);
        int i0 = 0, i2 = 2;                                   // the first of the smallest, the last of the largest: never the same entry
        if (a[1][1] < a[0][0]) i0 = 1;
        if (a[2][2] < mls_pick(i0, a[0][0], a[1][1], a[2][2])) i0 = 2;
        if (a[1][1] > a[2][2]) i2 = 1;
        if (a[0][0] > mls_pick(i2, a[0][0], a[1][1], a[2][2])) i2 = 0;
        const int i1 = 3 - i0 - i2;
        const double l0 = mls_pick(i0, a[0][0], a[1][1], a[2][2]), l1 = mls_pick(i1, a[0][0], a[1][1], a[2][2]),
                     l2 = mls_pick(i2, a[0][0], a[1][1], a[2][2]);
        if (l1 > fmax(MLS_RANK_TOL * l2, MLS_ROUNDING_FLOOR * W * h * h)) {
            double nx = mls_pick(i0, ev[0][0], ev[0][1], ev[0][2]), ny = mls_pick(i0, ev[1][0], ev[1][1], ev[1][2]),
                   nz = mls_pick(i0, ev[2][0], ev[2][1], ev[2][2]);
            bool flip;
            if (nrm) flip = (wnx * nx + wny * ny) + wnz * nz < 0.0;
            else {
                const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
                double big = nx, abig = ax;
                if (ay > abig) { big = ny; abig = ay; }
                if (az > abig) { big = nz; abig = az; }
                flip = big < 0.0;
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
            const double mn = (mx * nx + my * ny) + mz * nz;
            const double ox = mn * nx, oy = mn * ny, oz = mn * nz;
            used = 1;
            px = q0 + ox; py = q1 + oy; pz = q2 + oz;
            onx = nx; ony = ny; onz = nz;
            var = l0 / ((l0 + l1) + l2);

            if (ORDER == 2) {
                const double ux = mls_pick(i1, ev[0][0], ev[0][1], ev[0][2]), uy = mls_pick(i1, ev[1][0], ev[1][1], ev[1][2]),
                             uz = mls_pick(i1, ev[2][0], ev[2][1], ev[2][2]);
                const double vx = mls_pick(i2, ev[0][0], ev[0][1], ev[0][2]), vy = mls_pick(i2, ev[1][0], ev[1][1], ev[1][2]),
                             vz = mls_pick(i2, ev[2][0], ev[2][1], ev[2][2]);
                const double inv_h = 1.0 / h;
                // ---- second walk: the upper triangle of sum w b b^T (row after row) and sum w b z, b = (1, x, y, x^2, x y, y^2) ----
                double A[21], rhs[6];
#pragma unroll
                for (int t = 0; t < 21; ++t) A[t] = 0.0;
#pragma unroll
                for (int t = 0; t < 6; ++t) rhs[t] = 0.0;
                knn_cells27(g, c, [&](int ci) {
                    knn_scan4(g.xyz, g.start[ci], g.end[ci], q, [&](int kk, float d2f) {
                        if (!(d2f <= r2)) return;
                        const double dx = (double)g.xyz[(int64_t)kk * 3] - q0, dy = (double)g.xyz[(int64_t)kk * 3 + 1] - q1,
                                     dz = (double)g.xyz[(int64_t)kk * 3 + 2] - q2;
                        const double w = exp(-((dx * dx + dy * dy) + dz * dz) * inv_s2);
                        const double rx = dx - ox, ry = dy - oy, rz = dz - oz;
                        const double x = ((rx * ux + ry * uy) + rz * uz) * inv_h, y = ((rx * vx + ry * vy) + rz * vz) * inv_h,
                                     z = ((rx * nx + ry * ny) + rz * nz) * inv_h;
                        const double b[6] = {1.0, x, y, x * x, x * y, y * y};
                        int t = 0;
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            const double wb = w * b[r];
#pragma unroll
                            for (int s = r; s < 6; ++s) A[t++] += wb * b[s];
                            rhs[r] += wb * z;
                        }
                    });
                    return true;
                });
                // ---- Cholesky A = L L^T, every pivot held against the largest diagonal entry ----
                double L[6][6];
                {
                    int t = 0;
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int s = r; s < 6; ++s) { L[s][r] = A[t]; L[r][s] = A[t]; ++t; }
                }
                double dmax = L[0][0];
#pragma unroll
                for (int r = 1; r < 6; ++r) dmax = fmax(dmax, L[r][r]);
                bool ok = true;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    double s = L[j][j];
#pragma unroll
                    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
                    if (!(s > MLS_RANK_TOL * dmax)) { ok = false; s = 1.0; }          // (the rest runs on, its result is not used)
                    const double d = sqrt(s);
                    L[j][j] = d;
#pragma unroll
                    for (int r = j + 1; r < 6; ++r) {
                        double t = L[r][j];
#pragma unroll
                        for (int k = 0; k < j; ++k) t -= L[r][k] * L[j][k];
                        L[r][j] = t / d;
                    }
                }
                if (ok) {
                    double yv[6], av[6];
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        double t = rhs[r];
#pragma unroll
                        for (int k = 0; k < r; ++k) t -= L[r][k] * yv[k];
                        yv[r] = t / L[r][r];
                    }
#pragma unroll
                    for (int r = 5; r >= 0; --r) {
                        double t = yv[r];
#pragma unroll
                        for (int k = r + 1; k < 6; ++k) t -= L[k][r] * av[k];
                        av[r] = t / L[r][r];
                    }
                    const double step = av[0] * h;
                    px = q0 + (ox + step * nx); py = q1 + (oy + step * ny); pz = q2 + (oz + step * nz);
                    double gx = (nx - av[1] * ux) - av[2] * vx, gy = (ny - av[1] * uy) - av[2] * vy, gz = (nz - av[1] * uz) - av[2] * vz;
                    const double gl = sqrt((gx * gx + gy * gy) + gz * gz);           // >= 1: u, v, n are orthonormal
                    onx = gx / gl; ony = gy / gl; onz = gz / gl;
                    const double fx = av[1], fy = av[2], fxx = 2.0 * av[3] * inv_h, fxy = av[4] * inv_h, fyy = 2.0 * av[5] * inv_h;
                    const double e = (1.0 + fx * fx) + fy * fy;
                    Kc = (fxx * fyy - fxy * fxy) / (e * e);
                    Hc = -(((1.0 + fy * fy) * fxx - 2.0 * fx * fy * fxy) + (1.0 + fx * fx) * fyy) / (2.0 * e * sqrt(e));
                    used = 2;
                }
            }
        }
    }
    pos_out[i * 3] = px; pos_out[i * 3 + 1] = py; pos_out[i * 3 + 2] = pz;
    nrm_out[i * 3] = onx; nrm_out[i * 3 + 1] = ony; nrm_out[i * 3 + 2] = onz;
    mean_out[i] = Hc;
    gauss_out[i] = Kc;
    var_out[i] = var;
    used_out[i] = (int8_t)used;
}

extern "C" int nksr_mls_project(const float* xyz_sorted, int64_t n_ref, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const float* normal_sorted, const float* query,
                                int64_t nq, float radius, double sigma, int order, int min_neighbors, double* position_out, double* normal_out,
                                double* mean_curvature_out, double* gaussian_curvature_out, double* variation_out, int32_t* count_out,
                                int8_t* order_used_out, void* stream) {
    if (nq < 0 || n_ref < 0) return nksr_set_error(NKSR_ERR_ARG, "mls project: negative size (nq=%lld, n_ref=%lld)", (long long)nq, (long long)n_ref);
    if (int rc = radius_grid_args("mls project", xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell, radius)) return rc;
    if (!(sigma > 0.0) || !(sigma < 1.7e308)) return nksr_set_error(NKSR_ERR_ARG, "mls project: sigma must be positive and finite");
    if (order != 1 && order != 2) return nksr_set_error(NKSR_ERR_ARG, "mls project: order must be 1 or 2 (got %d)", order);
    if (min_neighbors < (order == 1 ? 3 : 6))
        return nksr_set_error(NKSR_ERR_ARG, "mls project: min_neighbors must be >= %d at order %d (got %d)", order == 1 ? 3 : 6, order, min_neighbors);
    if (!query && nq > n_ref) return nksr_set_error(NKSR_ERR_ARG, "mls project: query NULL (the cloud itself) with nq = %lld > n_ref = %lld", (long long)nq, (long long)n_ref);
    if (nq > 0 && (!position_out || !normal_out || !mean_curvature_out || !gaussian_curvature_out || !variation_out || !count_out || !order_used_out))
        return nksr_set_error(NKSR_ERR_ARG, "mls project: NULL output arrays");
    if (nq == 0) return NKSR_OK;
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    const double h = (double)radius, inv_s2 = 1.0 / (sigma * sigma);
    if (order == 1)
        hipLaunchKernelGGL(k_mls_project<1>, dim3(nksr_blocks(nq, 128)), dim3(128), 0, (hipStream_t)stream, g, normal_sorted, query, nq,
                           radius * radius, h, inv_s2, min_neighbors, position_out, normal_out, mean_curvature_out, gaussian_curvature_out,
                           variation_out, count_out, order_used_out);
    else
        hipLaunchKernelGGL(k_mls_project<2>, dim3(nksr_blocks(nq, 128)), dim3(128), 0, (hipStream_t)stream, g, normal_sorted, query, nq,
                           radius * radius, h, inv_s2, min_neighbors, position_out, normal_out, mean_curvature_out, gaussian_curvature_out,
                           variation_out, count_out, order_used_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
