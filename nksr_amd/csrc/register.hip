// Rigid registration of point clouds (nksr_amd/register.py: cloud.icp): the pass an ICP iteration consists of.
//
//   k_icp_accumulate<METHOD>  nksr_icp_accumulate: one lane per source point -- transform (fp64), nearest target point within the radius
//                             (the 27 cells of a PointGrid with cell >= radius, knn_cells27 + knn_scan4 of knn_dev.h, fp32
//                             knn_d2 decides, ties go to the lowest caller index), then the terms of the normal equations in fp64:
//                             the moment sums of Kabsch (METHOD 0, point-to-point) or J J^T, J r of the linearised point-to-plane
//                             error (METHOD 1).  One row of partial sums per workgroup.
//   k_icp_reduce              nksr_icp_reduce: the column sums of those rows, one workgroup.
//
// Every sum is taken in a fixed order -- the 64 lanes of a wavefront by a butterfly (both partners add the same two numbers, so all
// lanes end with the same bits), the wavefronts of a block in wave order, the rows in row order -- and nothing is accumulated with
// atomics: the same call gives the same bits.  A lane owns ONE point, so the "accumulators" are that point's terms, formed once after
// the search (30 doubles for the plane method) and handed to the butterfly one after the other; the search itself keeps a distance,
// an index and twelve coordinates.  The terms are formed without fused multiply-adds, in the order include/nksr_hip.h states: a host
// restatement in plain fp64 arithmetic gets every term to the last bit, and differs from the sums by the summation order alone.
#include "common.h"
#include "icp_dev.h"
#include "knn_dev.h"

static_assert(NKSR_ICP_PT_PQ + 9 <= NKSR_ICP_FIELDS && NKSR_ICP_PL_JJ + 21 == NKSR_ICP_PL_JR && NKSR_ICP_PL_JR + 6 == NKSR_ICP_PL_RR &&
              NKSR_ICP_PL_RR < NKSR_ICP_FIELDS, "layout of the sums");

template <int METHOD>
__global__ void __launch_bounds__(NKSR_ICP_BLOCK) k_icp_accumulate(KnnGrid g, const int64_t* __restrict__ perm, const float* __restrict__ nrm,
                                                                   const float* __restrict__ src, int64_t n, const double* __restrict__ T,
                                                                   const double* __restrict__ centre, float r2, int64_t* __restrict__ corr,
                                                                   double* __restrict__ partials) {
    constexpr int NF = METHOD == 0 ? NKSR_ICP_PT_PQ + 9 : NKSR_ICP_PL_RR + 1;          // the fields this method fills
    const int64_t i = (int64_t)blockIdx.x * NKSR_ICP_BLOCK + threadIdx.x;
    double term[NKSR_ICP_FIELDS];
#pragma unroll
    for (int f = 0; f < NKSR_ICP_FIELDS; ++f) term[f] = 0.0;
    if (i < n) {
        const float s[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
        double p[3];
        icp_transform(T, s, p);
        const float q[3] = {(float)p[0], (float)p[1], (float)p[2]};          // the search runs on the rounded point
        // outside the key range (or not finite: the comparison fails) there is no cell to look up, and no correspondence
        const float lim = (float)((1 << 20) - 8);
        const bool in_range = fabsf(__fmul_rn(q[0], g.inv_cell)) < lim && fabsf(__fmul_rn(q[1], g.inv_cell)) < lim &&
                              fabsf(__fmul_rn(q[2], g.inv_cell)) < lim;
        int best = -1;
        float bd = r2;
        if (in_range) {
            int c[3];
            cell_of(g, q, c);
            // nearer wins; AT the best distance so far the first candidate (d2 == r2 counts) or the lower caller index
            auto consider = [&](int kk, float d2) {
                if (d2 < bd || (d2 == bd && (best < 0 || perm[kk] < perm[best]))) { bd = d2; best = kk; }
            };
            knn_cells27(g, c, [&](int ci) {
                knn_scan4(g.xyz, g.start[ci], g.end[ci], q, consider);
                return true;
            });
        }
        corr[i] = best >= 0 ? perm[best] : (int64_t)-1;
        if (best >= 0) {
            const double qd[3] = {(double)g.xyz[(int64_t)best * 3], (double)g.xyz[(int64_t)best * 3 + 1], (double)g.xyz[(int64_t)best * 3 + 2]};
            const double c3[3] = {centre[0], centre[1], centre[2]};
            icp_terms<METHOD>(p, qd, METHOD ? nrm + (int64_t)best * 3 : nullptr, c3, term);
        }
    }
    // every lane of the block from here on (lanes past the end and lanes without a correspondence carry zeros)
    block_row_sums<NF, NKSR_ICP_FIELDS>(term, partials);
}

// column sums of the rows: thread t takes field t % FIELDS of the rows t / FIELDS, + slices, + 2 slices ... in row order; the
// slices of a field are then added in slice order.  (1024 lanes = 32 slices: the one workgroup has 1 MB of rows to read at 1 M points)
#define ICP_REDUCE_BLOCK 1024
#define ICP_REDUCE_SLICES (ICP_REDUCE_BLOCK / NKSR_ICP_FIELDS)
__global__ void __launch_bounds__(ICP_REDUCE_BLOCK) k_icp_reduce(const double* __restrict__ partials, int64_t nrows, double* __restrict__ out) {
    __shared__ double s[ICP_REDUCE_SLICES][NKSR_ICP_FIELDS];
    const int f = threadIdx.x % NKSR_ICP_FIELDS, slice = threadIdx.x / NKSR_ICP_FIELDS;
    double acc = 0.0;
    for (int64_t r = slice; r < nrows; r += ICP_REDUCE_SLICES) acc += partials[r * NKSR_ICP_FIELDS + f];
    s[slice][f] = acc;
    __syncthreads();
    if (slice == 0) {
        double v = 0.0;
        for (int k = 0; k < ICP_REDUCE_SLICES; ++k) v += s[k][f];
        out[f] = v;
    }
}

extern "C" int nksr_icp_accumulate(const float* xyz_sorted, int64_t n_ref, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                                   const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const int64_t* perm, const float* normal_sorted,
                                   const float* source, int64_t n_src, const double* transform, const double* centre, float radius, int method,
                                   int64_t* corr_out, double* partials_out, void* stream) {
    if (n_src < 0 || n_ref < 0) return nksr_set_error(NKSR_ERR_ARG, "icp accumulate: negative size (n_src=%lld, n_ref=%lld)", (long long)n_src, (long long)n_ref);
    if (int rc = radius_grid_args("icp accumulate", xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell, radius, n_src == 0)) return rc;
    if (method != 0 && method != 1) return nksr_set_error(NKSR_ERR_ARG, "icp accumulate: method must be 0 (point) or 1 (plane), got %d", method);
    if (n_src == 0) return NKSR_OK;
    if (!perm || !source || !transform || !centre) return nksr_set_error(NKSR_ERR_ARG, "icp accumulate: NULL perm / source / transform / centre");
    if (method == 1 && !normal_sorted) return nksr_set_error(NKSR_ERR_ARG, "icp accumulate: the plane method needs the target's normals");
    if (!corr_out || !partials_out) return nksr_set_error(NKSR_ERR_ARG, "icp accumulate: NULL output arrays");
    KnnGrid g = make_grid(xyz_sorted, start, end, hkeys, hvals, hcap, cell, inv_cell);
    const dim3 grid(nksr_blocks(n_src, NKSR_ICP_BLOCK)), block(NKSR_ICP_BLOCK);
    if (method == 0)
        hipLaunchKernelGGL(k_icp_accumulate<0>, grid, block, 0, (hipStream_t)stream, g, perm, normal_sorted, source, n_src, transform, centre,
                           radius * radius, corr_out, partials_out);
    else
        hipLaunchKernelGGL(k_icp_accumulate<1>, grid, block, 0, (hipStream_t)stream, g, perm, normal_sorted, source, n_src, transform, centre,
                           radius * radius, corr_out, partials_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_icp_reduce(const double* partials, int64_t nrows, double* sums_out, void* stream) {
    if (nrows < 0) return nksr_set_error(NKSR_ERR_ARG, "icp reduce: negative size");
    if (!partials || !sums_out) return nksr_set_error(NKSR_ERR_ARG, "icp reduce: NULL arrays");
    hipLaunchKernelGGL(k_icp_reduce, dim3(1), dim3(ICP_REDUCE_BLOCK), 0, (hipStream_t)stream, partials, nrows, sums_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
