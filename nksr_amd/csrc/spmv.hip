// The CSR SpMV, the roofline kernel of this project:
//   algorithmic bytes per launch  B_spmv = 8*nnz + 12*M + 4   (fp32 vals, int32 cols/rowptr)
// This file and spmv.h are all that build.kernel_hash('spmv') covers besides common.h: the counter records under profiles/ are keyed
// to the SpMV's own code, so the conjugate-gradient loop (csrc/pcg.hip) and the coarse-level block (csrc/cheb.hip) include nothing
// from here but spmv.h, and this file includes nothing of theirs.
#include "common.h"
#include "spmv.h"

#define PCG_BLOCK 256           // threads per workgroup, as in the conjugate-gradient kernels (csrc/pcg_dev.h, which this file does not see)
#define PCG_MAX_BLOCKS 2048

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- SpMV ---------------------------------------------------------------------------------------
// nnz-balanced streaming CSR SpMV.  The (col,val) stream is cut into chunks of CHUNK entries
// regardless of row boundaries (rows range from ~30 to several thousand entries: a coarse voxel
// couples to every fine voxel under its support), so every workgroup moves the same number of
// bytes with perfectly coalesced wide loads, ~32 KiB in flight per workgroup, ~8 workgroups per CU.
// Products go to LDS; each wavefront then reduces whole row segments from LDS (butterfly), writing y
// for rows that START in the chunk and one carry per chunk for the row that started earlier.  A tiny
// fix-up kernel adds the carries in chunk order, so the result is deterministic.  x gathers hit L2
// (Morton-ordered unknowns).
//
// Two physical layouts (nksr_hip.h, col_format), both interleaved so that component j of the load of
// lane l is logical entry 64 j + l of its tile -- every gather instruction covers 64 CONSECUTIVE
// entries of the stream:
//   format 0: EPL = 4 entries per lane, 256-entry tiles, int32 columns (16 + 16 bytes per lane)
//   format 1: EPL = 3 entries per lane, 192-entry tiles, three 21-bit columns packed in one 64-bit
//             word (8 + 12 bytes per lane): 6.67 instead of 8 bytes per entry, M <= 2^21.
// Storage is zero-padded (column 0, value 0) to a multiple of the chunk size: no bounds checks.
// The (col, val) stream is read with the non-temporal hint (round 3): it is touched once, and without the hint it pushed x out of the
// 4 MB L2 of every XCD (x is 4.5 MB at the bench workload): 589 -> 559 us per application, 0.639 -> 0.673 of 8 TB/s on the same box
// (VARIANT 2 = plain loads, kept for the comparison; VARIANT 1 = no gather: 465 us = what the stream alone allows).
template <int EPL> struct SpmvFmt {
    static constexpr int TILE = 64 * EPL;
    static constexpr int QUAD = PCG_BLOCK * EPL;          // entries per workgroup-wide load
    static constexpr int QUADS = EPL == 4 ? 4 : 6;
    static constexpr int CHUNK = QUADS * QUAD;            // 4096 / 4608
};
#define SPMV_CHUNK_MIN 4096
static int spmv_chunk(int fmt) { return fmt == 1 ? SpmvFmt<3>::CHUNK : SpmvFmt<4>::CHUNK; }

__global__ void k_spmv_plan(const int32_t* __restrict__ rowptr, int M, int64_t nnz, int nchunks, int chunk,
                            int32_t* __restrict__ chunk_row) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nchunks) return;
    if (b == nchunks) { chunk_row[b] = M; return; }
    // row containing entry b*CHUNK: last r with rowptr[r] <= k
    const int64_t k = (int64_t)b * chunk;
    int lo = 0, hi = M;  // invariant: rowptr[lo] <= k < rowptr[hi]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if ((int64_t)rowptr[mid] <= k) lo = mid; else hi = mid;
    }
    chunk_row[b] = lo;
}

struct f32x3_u { float x, y, z; } __attribute__((packed, aligned(4)));
typedef int spmv_v4i __attribute__((ext_vector_type(4)));
typedef float spmv_v4f __attribute__((ext_vector_type(4)));

template <int EPL, int VARIANT>
__global__ void __launch_bounds__(PCG_BLOCK) k_spmv(const int32_t* __restrict__ rowptr, const void* __restrict__ cols_,
                                                    const float* __restrict__ vals, int M, int nnz, int nchunks,
                                                    const int32_t* __restrict__ chunk_row, const float* __restrict__ x,
                                                    float* __restrict__ y, float* __restrict__ carry,
                                                    int32_t* __restrict__ carry_row, const int* __restrict__ done) {
    if (done && *done) return;
    typedef SpmvFmt<EPL> F;
    __shared__ __attribute__((aligned(16))) float prod[F::CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // chunks are dealt round-robin to the workgroups (a contiguous range per workgroup measured 8 %
    // slower: the concurrently active chunks then crowd the same HBM channels)
    // (round 3: giving every XCD one contiguous eighth of the chunks -- so that the x entries it gathers fit its own 4 MB L2 --
    // measured 6 % slower than round-robin, with or without the streaming hint below: same channel crowding)
    for (int b = blockIdx.x; b < nchunks; b += gridDim.x) {
        const int base = b * F::CHUNK;
        const int end = (base + F::CHUNK < nnz) ? base + F::CHUNK : nnz;
        // row pointers of the rows this wavefront will reduce (lane j: row r_first + wave + 4 j), fetched
        // now so that their latency hides behind the stream loads instead of stalling the row loop
        const int r_first = chunk_row[b], r_lim = chunk_row[b + 1];      // r_lim: row holding entry `end` (or M)
        int pre0 = 0x7fffffff, pre1 = 0x7fffffff;
        {
            const int r = r_first + wave + (PCG_BLOCK / 64) * lane;
            if (r <= r_lim && r < M) { pre0 = rowptr[r]; pre1 = rowptr[r + 1]; }
        }
        int c[F::QUADS][EPL];
        float v[F::QUADS][EPL];
#pragma unroll
        for (int q = 0; q < F::QUADS; ++q) {
            const int64_t g = (int64_t)(base + q * F::QUAD) / EPL + tid;       // lane slot (EPL entries)
            if (EPL == 4) {
                int4 ci;
                float4 vi;
                if (VARIANT != 2) {
                    const spmv_v4i cn = __builtin_nontemporal_load(reinterpret_cast<const spmv_v4i*>(cols_) + g);
                    const spmv_v4f vn = __builtin_nontemporal_load(reinterpret_cast<const spmv_v4f*>(vals) + g);
                    ci = make_int4(cn.x, cn.y, cn.z, cn.w); vi = make_float4(vn.x, vn.y, vn.z, vn.w);
                } else { ci = reinterpret_cast<const int4*>(cols_)[g]; vi = reinterpret_cast<const float4*>(vals)[g]; }
                c[q][0] = ci.x; c[q][1] = ci.y; c[q][2] = ci.z; c[q][EPL - 1] = ci.w;
                v[q][0] = vi.x; v[q][1] = vi.y; v[q][2] = vi.z; v[q][EPL - 1] = vi.w;
            } else {
                const unsigned long long pk = VARIANT != 2 ? __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(cols_) + g)
                                                           : reinterpret_cast<const unsigned long long*>(cols_)[g];
                f32x3_u vi;
                if (VARIANT != 2) {
                    const float* vp = vals + 3 * g;
                    vi.x = __builtin_nontemporal_load(vp); vi.y = __builtin_nontemporal_load(vp + 1); vi.z = __builtin_nontemporal_load(vp + 2);
                } else vi = reinterpret_cast<const f32x3_u*>(vals)[g];
                c[q][0] = (int)(pk & 0x1FFFFFull); c[q][1] = (int)((pk >> 21) & 0x1FFFFFull); c[q][2] = (int)((pk >> 42) & 0x1FFFFFull);
                v[q][0] = vi.x; v[q][1] = vi.y; v[q][2] = vi.z;
            }
        }
#pragma unroll
        for (int q = 0; q < F::QUADS; ++q) {
            float* pt = prod + q * F::QUAD + wave * F::TILE + lane;
#pragma unroll
            for (int j = 0; j < EPL; ++j)
                pt[64 * j] = v[q][j] * (VARIANT == 1 ? (float)c[q][j] : x[c[q][j]]);   // VARIANT 1: probe without the gather
        }
        __syncthreads();
        if (tid == 0 && pre0 >= base) carry_row[b] = -1;   // no row continues into this chunk
        int j = 0;
        for (int r = r_first + wave; r <= r_lim && r < M; r += PCG_BLOCK / 64, ++j) {
            int p0, p1;
            if (j < 64) { p0 = __builtin_amdgcn_readlane(pre0, j); p1 = __builtin_amdgcn_readlane(pre1, j); }
            else { p0 = rowptr[r]; p1 = rowptr[r + 1]; }
            if (p0 >= end) break;                          // row r_lim starts exactly at `end`: next chunk's
            const int k0 = p0 > base ? p0 : base, k1 = p1 < end ? p1 : end;
            float s = 0.f;
            for (int k = k0 + lane; k < k1; k += 64) s += prod[k - base];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) {
                if (p0 >= base) y[r] = s;
                else { carry[b] = s; carry_row[b] = r; }
            }
        }
        __syncthreads();
    }
}

// three int32 columns (< 2^21) of one lane slot -> one 64-bit word (format 1)
__global__ void k_pack_cols21(const int32_t* __restrict__ cols32, int64_t nslots, unsigned long long* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nslots) return;
    const unsigned long long a = (unsigned)cols32[3 * g], b = (unsigned)cols32[3 * g + 1], c = (unsigned)cols32[3 * g + 2];
    out[g] = a | (b << 21) | (c << 42);
}

// adds the per-chunk carries to y in chunk order (one thread per run of equal rows)
__global__ void k_spmv_fixup(int nchunks, const float* __restrict__ carry, const int32_t* __restrict__ carry_row,
                             float* __restrict__ y, const int* __restrict__ done) {
    if (done && *done) return;
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nchunks) return;
    const int r = carry_row[b];
    if (r < 0) return;
    if (b > 0 && carry_row[b - 1] == r) return;   // not the head of the run
    float s = 0.f;
    for (int j = b; j < nchunks && carry_row[j] == r; ++j) s += carry[j];
    y[r] += s;
}

// ---- SpMV plan / workspace ------------------------------------------------------------------------
static int spmv_nchunks(int64_t nnz, int fmt) { return (int)((nnz + spmv_chunk(fmt) - 1) / spmv_chunk(fmt)); }

extern "C" size_t nksr_spmv_workspace_bytes(int64_t nnz) {
    size_t nc = (size_t)((nnz + SPMV_CHUNK_MIN - 1) / SPMV_CHUNK_MIN);   // enough for either format
    return align_up((nc + 1) * sizeof(int32_t), 256) + 2 * align_up(nc * sizeof(float), 256) + 256;
}

SpmvPlan carve_spmv(void* ws, int64_t nnz, int fmt) {
    SpmvPlan p;
    p.nchunks = spmv_nchunks(nnz, fmt);
    char* c = (char*)ws;
    p.chunk_row = (int32_t*)c; c += align_up(((size_t)p.nchunks + 1) * sizeof(int32_t), 256);
    p.carry = (float*)c; c += align_up((size_t)p.nchunks * sizeof(float), 256);
    p.carry_row = (int32_t*)c;
    return p;
}

static int spmv_grid(int nchunks) {
    return nchunks < 1 ? 1 : (nchunks > PCG_MAX_BLOCKS ? PCG_MAX_BLOCKS : nchunks);
}

static int check_format(int col_format, int M) {
    if (col_format != 0 && col_format != 1) return nksr_set_error(NKSR_ERR_ARG, "col_format must be 0 or 1");
    if (col_format == 1 && M > (1 << 21)) return nksr_set_error(NKSR_ERR_CAPACITY, "col_format 1 packs 21-bit columns: M = %d > 2^21", M);
    return NKSR_OK;
}

extern "C" int nksr_spmv_plan(const int32_t* rowptr, int32_t M, int64_t nnz, int col_format, void* workspace, void* stream) {
    if (M <= 0 || nnz <= 0) return NKSR_OK;
    if (nnz >= ((int64_t)1 << 31) - SpmvFmt<3>::CHUNK) return nksr_set_error(NKSR_ERR_CAPACITY, "nnz exceeds int32");
    if (int rc = check_format(col_format, M)) return rc;
    SpmvPlan p = carve_spmv(workspace, nnz, col_format);
    hipLaunchKernelGGL(k_spmv_plan, dim3(nksr_blocks(p.nchunks + 1, 256)), dim3(256), 0, (hipStream_t)stream, rowptr, M, nnz,
                       p.nchunks, spmv_chunk(col_format), p.chunk_row);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_pack_cols21(const int32_t* cols32, int64_t n_padded, uint64_t* packed_out, void* stream) {
    if (n_padded % SpmvFmt<3>::TILE) return nksr_set_error(NKSR_ERR_ARG, "n_padded must be a multiple of %d", SpmvFmt<3>::TILE);
    const int64_t nslots = n_padded / 3;
    if (nslots > 0) {
        hipLaunchKernelGGL(k_pack_cols21, dim3(nksr_blocks(nslots, 256)), dim3(256), 0, (hipStream_t)stream, cols32, nslots,
                           (unsigned long long*)packed_out);
        NKSR_CHECK_LAUNCH();
    }
    return NKSR_OK;
}

static int g_spmv_variant = 0;
extern "C" int nksr_spmv_set_variant(int v) { g_spmv_variant = v; return NKSR_OK; }

int launch_spmv(const int32_t* rowptr, const void* cols, const float* vals, int M, int64_t nnz, int fmt, const SpmvPlan& p,
                const float* x, float* y, const int* done, hipStream_t st) {
#define SPMV_LAUNCH(E, V) hipLaunchKernelGGL((k_spmv<E, V>), dim3(spmv_grid(p.nchunks)), dim3(PCG_BLOCK), 0, st, rowptr, cols, vals, M, (int)nnz, \
                       p.nchunks, p.chunk_row, x, y, p.carry, p.carry_row, done)
    if (fmt == 1) { if (g_spmv_variant == 1) SPMV_LAUNCH(3, 1); else if (g_spmv_variant == 2) SPMV_LAUNCH(3, 2); else SPMV_LAUNCH(3, 0); }
    else { if (g_spmv_variant == 1) SPMV_LAUNCH(4, 1); else if (g_spmv_variant == 2) SPMV_LAUNCH(4, 2); else SPMV_LAUNCH(4, 0); }
    hipLaunchKernelGGL(k_spmv_fixup, dim3(nksr_blocks(p.nchunks, 256)), dim3(256), 0, st, p.nchunks, p.carry, p.carry_row, y, done);
    return 0;
}

extern "C" int nksr_spmv_csr(const int32_t* rowptr, const void* cols, const float* vals, int32_t M, int64_t nnz, int col_format,
                             const float* x, float* y, void* workspace, void* stream) {
    if (M <= 0) return NKSR_OK;
    if (!workspace) return nksr_set_error(NKSR_ERR_ARG, "workspace is NULL (run nksr_spmv_plan first)");
    if (int rc = check_format(col_format, M)) return rc;
    SpmvPlan p = carve_spmv(workspace, nnz, col_format);
    launch_spmv(rowptr, cols, vals, M, nnz, col_format, p, x, y, nullptr, (hipStream_t)stream);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

void spmv_bytes(int M, int64_t nnz, int fmt, double* alg, double* phys) {
    *alg = 8.0 * (double)nnz + 12.0 * (double)M + 4.0;
    const int chunk = spmv_chunk(fmt);
    const double npad = (double)((nnz + chunk - 1) / chunk) * chunk;
    *phys = (fmt == 1 ? (4.0 + 8.0 / 3.0) : 8.0) * npad + 12.0 * (double)M + 4.0;
}
