/* nksr_hip.h -- C-ABI of the MI355X-native NKSR solve-time hot path.
 *
 * Drop-in boundary.  The reference's native boundary is the
 * compiled `_C` module inside the un-vendored `nksr` wheel (README.md:46), reached
 * through the Python surface evidenced at examples/recons_simple.py:25-27,
 * models/nksr_net.py:57-62,91-112 and models/loss.py:189-198.  Each entry point
 * below names the reference-side call it serves.  Conventions:
 *   - plain device pointers + sizes; the caller (Python/torch) owns every buffer
 *   - `stream` is a hipStream_t passed as void*
 *   - return 0 on success, negative on error; nksr_last_error() gives the message
 *   - no hidden host synchronisation unless the doc comment says "syncs"
 */
#ifndef NKSR_HIP_H
#define NKSR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NKSR_MAX_DEPTH 6
#define NKSR_OK 0
#define NKSR_ERR_ARG (-1)
#define NKSR_ERR_HIP (-2)
#define NKSR_ERR_CAPACITY (-3)

const char* nksr_last_error(void);
int nksr_version(void);

/* ---- one level of the sparse voxel hierarchy (SparseFeatureHierarchy.grids[d],
 *      models/nksr_net.py:57-62, models/loss.py:33-46) ------------------------------- */
typedef struct {
    int32_t n;                 /* active voxels, canonical order = ascending Morton key */
    int32_t offset;            /* first unknown index of this level in alpha            */
    const int64_t* keys;       /* [n] sorted Morton keys                                */
    const int32_t* ijk;        /* [n,3]                                                 */
    const int32_t* nbr;        /* [n,27] neighbour voxel index or -1                    */
    const int64_t* hkeys;      /* open-addressing hash: keys (-1 = empty)               */
    const int32_t* hvals;      /*                      values                           */
    int32_t hcap;              /* capacity (power of two)                               */
    const float* feat;         /* [n,K] basis features                                  */
    const float* psi;          /* [n,K] phi_d(c_j)                                      */
    const float* mlp;          /* interpolator weights W1[H,K] b1[H] W2[H,H] b2[H] W3[K,H] b3[K] */
} nksr_level_t;

typedef struct {
    int32_t depth, kdim, hidden;
    float inv_w0;              /* fp32 reciprocal of the finest voxel size              */
    nksr_level_t lv[NKSR_MAX_DEPTH];
} nksr_hier_t;

/* ---- device primitives (rocPRIM-backed; tmp==NULL -> size query) --------------------- */
int nksr_sort_keys_u64(void* tmp, size_t* tmp_bytes, const uint64_t* in, uint64_t* out, int64_t n,
                       int begin_bit, int end_bit, void* stream);
int nksr_sort_pairs_u64_u32(void* tmp, size_t* tmp_bytes, const uint64_t* kin, uint64_t* kout,
                            const uint32_t* vin, uint32_t* vout, int64_t n, int begin_bit, int end_bit, void* stream);
int nksr_unique_u64(void* tmp, size_t* tmp_bytes, const uint64_t* in, uint64_t* out, int64_t* d_count,
                    int64_t n, void* stream);
int nksr_exclusive_sum_i32(void* tmp, size_t* tmp_bytes, const int32_t* in, int32_t* out, int64_t n, void* stream);
int nksr_exclusive_sum_i64(void* tmp, size_t* tmp_bytes, const int64_t* in, int64_t* out, int64_t n, void* stream);
/* The run table of n SORTED keys (compared unsigned): the edges of a mesh, the clusters of a simplification, the voxels of a cloud.
 * Keys >= none_from belong to no run (sorted, they are a tail); pass UINT64_MAX for "every key counts" -- the all-ones key is then
 * never in a run.  Position i HEADS a run when its key is < none_from and differs from its predecessor's, or when i = 0.
 * Sequence: nksr_run_counts_u64, nksr_exclusive_sum_i64 over the [blocks + 1] counts, (read n_runs = the scan's last entry),
 * nksr_run_table_u64.  n < 2^32 (the starts are uint32); with run_of_out n_runs < 2^31.
 * block_counts [nksr_run_blocks(n) + 1] = heads per block of 256 positions, then a 0.
 * start_out [n_runs + 1] = the sorted position of every run's head, and at [n_runs] the position of the first key >= none_from, or n
 * (0 for n = 0 and when no key is in a run); run_key_out [n_runs] or NULL = the runs' keys; run_of_out [n] or NULL = the run of every
 * position, -1 for a key >= none_from. */
int64_t nksr_run_blocks(int64_t n);                        /* ceil(n / 256), 0 for n <= 0 */
int nksr_run_counts_u64(const uint64_t* keys_sorted, int64_t n, uint64_t none_from, int64_t* block_counts, void* stream);
int nksr_run_table_u64(const uint64_t* keys_sorted, int64_t n, uint64_t none_from, const int64_t* block_offsets, int64_t n_runs,
                       uint32_t* start_out, uint64_t* run_key_out, int32_t* run_of_out, void* stream);

/* ---- hierarchy build/query (SparseFeatureHierarchy.build_point_splatting,
 *      models/nksr_net.py:62; grids[d].active_grid_coords models/loss.py:36) ------------ */
/* mode 0: 8 nearest voxel centres per point (encoder hierarchy); mode 1: containing
 * cell + 26 neighbours (decoder structure rule).  keys_out has n*8 / n*27 entries. */
int nksr_splat_keys(const float* xyz, int64_t n, float inv_w0, int level, int mode, int64_t* keys_out, void* stream);
/* Same footprints generated from the unique level-`level` CELLS that hold points instead of from every
 * point: mode 0 -> 8 keys per cell at level+1 (the level-(l+1) half index of a point is its level-l cell
 * index), mode 1 -> 27 keys per cell at the same level. */
int nksr_cell_footprint_keys(const int64_t* cell_keys, int64_t nc, int level, int mode, int64_t* keys_out, void* stream);
/* Axis-aligned bounding box of a cloud (the host side of detail_level / chunk_size needs it: NKSR-USAGE.md:129-137):
 * out6 = (min x, y, z, max x, y, z), exact; out6[0] = NaN when any coordinate is NaN / infinite (the readback of the box is the
 * finiteness check of the input); work: nksr_bbox_work_floats() floats of scratch. */
int nksr_bbox(const float* xyz, int64_t n, float* work, float* out6, void* stream);
int64_t nksr_bbox_work_floats(void);
/* The same key streams (xyz != NULL: nksr_splat_keys; cell_keys != NULL: nksr_cell_footprint_keys; exactly one of them) with the
 * duplicates inside each workgroup's range of Morton-ordered elements (several thousand of them) mostly removed (LDS hash set,
 * emitted and cleared when it fills up and at the end of the range): the multiset differs, the SET of keys
 * is the same, so sort + unique behind it give the identical level.  keys_out: room for n * (8 | 27) keys; *count_out (device)
 * = number of keys written, in no particular order.  mode 2 (cell_keys, level 0): the corner keys of nksr_cell_corner_keys;
 * mode 3 (cell_keys, level 0): cell_keys IS the stream (n non-negative keys, e.g. the edge keys of nksr_mc_emit). */
int nksr_footprint_keys_dedup(const float* xyz, const int64_t* cell_keys, int64_t n, float inv_w0, int level, int mode,
                              int64_t* keys_out, int64_t* count_out, void* stream);
/* Morton key of the level-0 cell containing each point. */
int nksr_point_keys(const float* xyz, int64_t n, float inv_w0, int64_t* keys_out, void* stream);
int nksr_decode_keys(const int64_t* keys, int64_t n, int level, int32_t* ijk_out, void* stream);
int nksr_encode_keys(const int32_t* ijk, int64_t n, int level, int64_t* keys_out, void* stream);
/* Open-addressing table Morton key -> value (the key's rank): hcap a power of two >= max(8, 2 n); hkeys must be pre-filled with 0xFF
 * bytes.  The eight children of a cell (keys equal above their low three bits) share one 64-byte line of hkeys; a collision moves to
 * another line (csrc/common.h: hash_slot / hash_next). */
int nksr_hash_build(const int64_t* keys, int32_t n, int64_t* hkeys, int32_t* hvals, int32_t hcap, void* stream);
int nksr_hash_query(const int64_t* q, int64_t nq, const int64_t* hkeys, const int32_t* hvals, int32_t hcap,
                    int32_t* idx_out, void* stream);
int nksr_build_nbr(const int32_t* ijk, int32_t n, int level, const int64_t* hkeys, const int32_t* hvals,
                   int32_t hcap, int32_t* nbr_out, void* stream);
/* The same table derived from the next-coarser level (every voxel's parent active): parent_idx [n] = index of voxel i's parent in
 * the coarse level (-1: none -- then the whole level falls back to the hash, decided on the device), coarse_nbr [n_coarse, 27],
 * work = 2 n_coarse + 1 int32, the first n_coarse and the last ZEROED by the caller.  Same result as nksr_build_nbr. */
int nksr_build_nbr_from_parent(const int32_t* ijk, const int64_t* keys, int32_t n, int level, const int64_t* hkeys, const int32_t* hvals,
                               int32_t hcap, const int32_t* parent_idx, const int32_t* coarse_nbr, int32_t n_coarse, int32_t* work,
                               int32_t* nbr_out, void* stream);
/* start/end of the sites (sorted level-0 Morton keys) that fall inside each level-d voxel */
int nksr_site_ranges(const int64_t* site_keys, int64_t ns, const int64_t* vox_keys, int32_t n, int level,
                     int32_t* start_out, int32_t* end_out, void* stream);

/* ---- trilinear splats (csrc/splat.hip: this one, nksr_splat_mean, nksr_splat_encode, nksr_splat_plane) ---- */
/* Trilinear splat (weighted sum + weight sum) of per-point features onto the voxels of one
 * level; points must be Morton-sorted with start/end = nksr_site_ranges of that level.
 * Point encoder skip path (network.encoder, models/nksr_net.py:73).
 * With n > 0 every array must be non-NULL (NKSR_ERR_ARG otherwise) AND the cloud must hold at least one point: the splats carry no
 * point count and read point 0 unconditionally.  An empty cloud is the caller's case (nn/network.py returns zeros without a launch). */
int nksr_splat_trilinear(const float* xyz_sorted, const float* feat_sorted, int C, const int32_t* start,
                         const int32_t* end, const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w,
                         float* out, float* wsum_out, void* stream);

/* ---- sparse feature-hierarchy network (network.encoder / network.unet, models/nksr_net.py:73-78;
 *      csrc/nn.hip; the splats: csrc/splat.hip).  C = unet.f_maps = 32 (configs/default/train.yaml:17-18).
 *      Every entry below checks its arguments before any launch: with n > 0 a NULL array is NKSR_ERR_ARG (a NULL pointer would pass
 *      the 16-byte alignment tests); the optional ones are named.  n <= 0 is NKSR_OK and touches nothing. --------------------- */
/* per-point MLP on [local cell coordinate - 1/2 (3), orientation feature (3)]:  W1 [C,6], W2 [C,C] */
int nksr_point_mlp(const float* xyz, const float* feat, int64_t n, float inv_w0, int C, const float* W1,
                   const float* b1, const float* W2, const float* b2, float* out, void* stream);
/* trilinear splat-MEAN of C-channel (1..64) point features onto one level (points Morton-sorted; at least one point, see
 * nksr_splat_trilinear) */
int nksr_splat_mean(const float* xyz_sorted, const float* feat_sorted, int C, const int32_t* start,
                    const int32_t* end, const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w, float* out,
                    void* stream);
/* The point encoder's two splats onto one level in ONE pass over the points: voxel_feat [n, 32] = nksr_splat_mean of the 32-channel
 * feat_sorted, and -- normal_sorted [N, 3] != NULL -- normal_sum [n, 3], weight_sum [n] = nksr_splat_trilinear of normal_sorted on the
 * same level, each bit for bit.  normal_sorted: optional (NULL: normal_sum / weight_sum are not touched and may be NULL). */
int nksr_splat_encode(const float* xyz_sorted, const float* feat_sorted, const float* normal_sorted, const int32_t* start,
                      const int32_t* end, const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w, float* voxel_feat,
                      float* normal_sum, float* weight_sum, void* stream);
/* 3x3x3 submanifold sparse convolution on the fp32 matrix cores: out = act(b + sum_s W[s]^T in[nbr[:,s]]
 * (+ residual)),  W [27, C, C]  in / W: 16-byte aligned (NKSR_ERR_ARG otherwise); bias / residual: optional (NULL). */
int nksr_sparse_conv3(const float* in, const int32_t* nbr, int32_t n, int C, const float* W, const float* bias,
                      const float* residual, int relu, float* out, void* stream);
/* Weight gradient of nksr_sparse_conv3 (training path, network.unet under autograd, models/nksr_net.py:74-78):
 * partial[chunk][s][ci][co] = sum over the chunk's voxels i of in[nbr[i][s]][ci] * gz[i][co]  (gz = output gradient through the
 * activation); nksr_conv3_wgrad_chunks(n) chunks, the caller adds them up (fixed order: deterministic). */
int64_t nksr_conv3_wgrad_chunks(int32_t n);
int nksr_conv3_wgrad(const float* in, const int32_t* nbr, int32_t n, int C, const float* gz, float* partial, void* stream);
/* mean over the children (contiguous Morton range start/end in the finer level) of every voxel */
int nksr_pool_children(const float* child_feat, const int32_t* start, const int32_t* end, int32_t n_parent, int C,
                       float* out, void* stream);
/* out[i] = (idx[i] >= 0 ? src[idx[i]] : 0) (+ add[i]) -- hierarchy transfer / parent->child up-sampling; add: optional (NULL) */
int nksr_gather_rows(const float* src, const int32_t* idx, int64_t n, int C, const float* add, float* out, void* stream);
/* per-voxel linear head: out [n, Cout] = in [n, 32] W^T + b,  1 <= Cout <= 32; b: optional (NULL) */
int nksr_linear(const float* in, int64_t n, int Cin, const float* W, const float* b, int Cout, float* out, void* stream);

/* ---- UDF mask branch: NeuralField(svh=udf_svh, decoder=network.udf_decoder, features=feat.udf_features)
 *      .set_level_set(2 * voxel_size)  (models/nksr_net.py:124-130; configs/carla/train.yaml:8-9) ---------- */
/* plane features of one level, out [n, 8] = (occupied, centroid offset xyz in voxel units, unit mean normal
 * xyz, 0): trilinear-weighted over the Morton-sorted points around every voxel (at least one point, see nksr_splat_trilinear);
 * NULL arrays with n > 0: NKSR_ERR_ARG */
int nksr_splat_plane(const float* xyz_sorted, const float* normal_sorted, const int32_t* start, const int32_t* end,
                     const int32_t* nbr, const int32_t* ijk, int32_t n, float inv_w, float* out, void* stream);
/* unsigned plane distance decoded from the 8 voxel centres around every query (1e30 where none is
 * occupied); only_unset != 0 keeps entries already decoded at a finer level.  NULL out, or NULL feat / xyz / hash table of a level
 * that has voxels, with n > 0: NKSR_ERR_ARG */
int nksr_udf_decode(const nksr_level_t* level, int level_index, const float* feat, const float* xyz, int64_t n,
                    float inv_w, float voxel_size, int only_unset, float* out, void* stream);

/* ---- neural kernel (KernelField, models/nksr_net.py:91-96) --------------------------- */
int nksr_voxel_psi(const float* feat, int32_t n, int kdim, int hidden, const float* mlp, float* psi_out, void* stream);
/* Dense-slot kernel rows at arbitrary sites.  val [n, L, 27] (may be NULL when only the gradient rows are
 * wanted); dval [n, 3, L, 27] (may be NULL).  approx!=0 drops the d(phi)/dx term (approx_kernel_grad, recons_waymo.py:33).  Every output is
 * multiplied by row_scale (the assembly takes rows pre-multiplied by sqrt(set weight), see nksr_assemble) -- or, when site_scale
 * (device, [n]) is given, by site_scale[i] instead: the sites of a batched chunk solve carry their own chunk's weight. */
int nksr_kernel_rows(const nksr_hier_t* h, const float* xyz, int64_t n, int approx, float row_scale, const float* site_scale,
                     int64_t level_stride, const int32_t* row_index, int32_t* row_cells, float* val, float* dval, void* stream);
/* level_stride > 0: LEVEL-MAJOR output, row (site i, component a) of level d at val / dval + ((d * level_stride + r_i + a) * 27) with
 * r_i = row_index ? row_index[i] : i * ncomp (ncomp = 1 for val, 3 for dval; ONE of val / dval when row_index is given) -- the layout
 * of the matrix-free solve (nksr_fused_op_t.rows_all): row_index lets several site sets share one Morton-ordered row list;
 * row_cells [L, level_stride] (may be NULL) receives the global unknown index of the level-d cell of every row written (-1 = none). */
/* The rows of BOTH site sets of the matrix-free operator in ONE pass over its merged row list (kernel_dim 4; KernelField.solve,
 * models/nksr_net.py:105-112 with fused_mode, examples/recons_waymo.py:33): rows_out [L][rows_total][27], row r of the list is
 * row_src[r] = (site << 2) | kind -- kind 0: the value row of position site `site` (xyz_pos), kind 1 + a: the d/dx_a row of normal
 * site `site` (xyz_nrm); row_src[r] < 0: a pad row (zeros, row_cells -1).  One launch writes every 128-byte line of rows_out whole
 * (a launch per set writes the interleaved rows as partial lines: 1.1 - 1.8 TB/s against 5.7); values bit-identical to
 * nksr_kernel_rows.  scale_* (device, per site) or row_scale_* as for nksr_kernel_rows; either set may be absent (xyz NULL).
 * sites < 2^29 per set. */
int nksr_kernel_rows_merged(const nksr_hier_t* h, const float* xyz_pos, const float* scale_pos, float row_scale_pos,
                            const float* xyz_nrm, const float* scale_nrm, float row_scale_nrm, int approx, const int32_t* row_src,
                            int64_t rows_total, const int32_t* row_cells, float* rows_out, void* stream);
/* row_cells [L][rows_total] (not NULL) is READ: nksr_row_cells_merged makes it in one pass with the probes of all levels in flight
 * together, and the row kernel's chain of dependent loads loses two links.
 * nksr_row_cells_merged: row_cells_out[d][r] = global unknown index of the level-d cell of row r's site, -1 = none (pad rows: -1). */
int nksr_row_cells_merged(const nksr_hier_t* h, const float* xyz_pos, const float* xyz_nrm, const int32_t* row_src, int64_t rows_total,
                          int32_t* row_cells_out, void* stream);
/* row_src of nksr_kernel_rows_merged from the sets' first rows: row_src[first_row[i] + c] = (i << 2) | (kind0 + c), c < ncomp
 * (ncomp 1, kind0 0: position sites; ncomp 3, kind0 1: normal sites).  The caller pre-fills row_src with -1. */
int nksr_row_sources(const int32_t* first_row, int64_t n, int ncomp, int kind0, int32_t* row_src, void* stream);
/* Rank-4 FACTORS of the same rows (kernel_dim 4 only; the matrix-free solve's row format since round 5, nksr_fused_op_t.fac_vec /
 * fac_pos): per row and level one 16-byte record instead of 27 slots.  grad == 0: one row per site, vec = phi_d(x) * scale.
 * grad != 0: FOUR rows per site -- a header row (vec = phi * scale) and one row per axis a (vec = d phi / d x_a * scale; 0 with
 * approx != 0).  Row r of site i = (row_index ? row_index[i] : i * rows_per_site) + q.  vec_out [L][level_stride][4],
 * pos_out [level_stride][4] = (x * inv_w0, kind bits), row_cells as for nksr_kernel_rows.  Rows of a site outside every active
 * cell of a level are 0 there. */
int nksr_kernel_factors(const nksr_hier_t* h, const float* xyz, int64_t n, int grad, int approx, float row_scale, const float* site_scale,
                        int64_t level_stride, const int32_t* row_index, int32_t* row_cells, float* vec_out, float* pos_out, void* stream);
/* f(x) (and gradient if grad_out != NULL): field.evaluate_f, models/loss.py:189-198.  alpha == NULL: the hierarchy's psi arrays
 * already hold alpha_j psi_j (one gather per neighbour instead of two).  A query outside every active cell of a level still sees the
 * voxels whose support covers it (hash lookups); active_only != 0 drops those levels instead -- the support of nksr_kernel_rows,
 * which is what the training path's backward differentiates. */
int nksr_evaluate_f(const nksr_hier_t* h, const float* alpha, const float* xyz, int64_t n, int approx, int active_only,
                    float* f_out, float* grad_out, void* stream);

/* ---- backward of the kernel rows w.r.t. theta = (basis features, interpolator weights): the training path, models/nksr_net.py:
 *      105-112 (loss -> solve_non_fused / evaluate_f -> network).  With per-row factors g_r[s] = a_r lam[col] + b_r alpha[col] the
 *      kernels ADD  dS/dtheta,  S = sum_r sum_s row_scale R_r[s] g_r[s]  (R = the rows of nksr_kernel_rows: value rows, or
 *      gradient rows with / without the d(phi)/dx term) to the caller's zero-initialised arrays.  coef_a / coef_b: [n] (value rows) or
 *      [n, 3] (gradient rows), either may be NULL (= 0; coef_a needs lam).  Floating-point atomics: reproducible to rounding. */
typedef struct {
    float* gfeat[NKSR_MAX_DEPTH]; /* [n_d, kdim] += through the trilinear stencil of the sites                                    */
    float* gpsi[NKSR_MAX_DEPTH];  /* [n_d, kdim] += dS/dpsi_j of the neighbour voxels (finish with nksr_voxel_psi_vjp)           */
    float* gmlp[NKSR_MAX_DEPTH];  /* packed interpolator weights of the level (W1 b1 W2 b2 W3 b3) +=                             */
} nksr_theta_grad_t;
int nksr_kernel_rows_vjp(const nksr_hier_t* h, const float* xyz, int64_t n, int grad_rows, int approx, float row_scale, const float* coef_a,
                         const float* coef_b, const float* alpha, const float* lam, const nksr_theta_grad_t* out, void* stream);
/* psi_j = f_j + MLP(f_j) (nksr_voxel_psi) backwards: gfeat_j += (d psi_j / d f_j)^T gpsi_j, gmlp += the weight cotangents */
int nksr_voxel_psi_vjp(const float* feat, int32_t n, int kdim, int hidden, const float* mlp, const float* gpsi, float* gfeat, float* gmlp,
                       void* stream);

/* ---- normal-equation assembly (KernelField.solve_non_fused, models/nksr_net.py:105-112) */
typedef struct {
    int64_t n;                 /* sites                                                */
    int32_t ncomp;             /* 1 (position rows, G) or 3 (gradient rows, Q)         */
    float weight;              /* weight of the set (>= 0).  For a bitwise symmetric matrix pass val / target
                                * pre-multiplied by sqrt(w) (nksr_kernel_rows row_scale) and weight = 1 */
    const float* val;          /* [n, ncomp, L, 27] dense-slot rows                    */
    const float* target;       /* [n, ncomp] right-hand side values or NULL (zero)     */
    const int32_t* start[NKSR_MAX_DEPTH]; /* per level: [n_d] site range per voxel     */
    const int32_t* end[NKSR_MAX_DEPTH];
    int64_t level_stride;      /* 0: val is site-major as above.  > 0: val is the LEVEL-MAJOR array of the matrix-free operator
                                * ([L, level_stride, 27], nksr_fused_op_t.rows_all) and site i owns the rows row_index[i] .. + ncomp */
    const int32_t* row_index;  /* [n] first row of every site (level-major layout; NULL = i * ncomp) */
    int64_t level_base;        /* level-major rows only: val STARTS at this level ([L - level_base, level_stride, 27]; the factor form of the
                                * operator keeps dense rows of its coarse levels only) -- the assembly must then be asked for levels >= level_base */
} nksr_siteset_t;

/* Structure pass.  Per row: rowcount = structural upper entries (column voxel exists, B-spline supports
 * overlap, col > row), crosscount = those of them whose column lies on a coarser level (only these are
 * mirrored), samelow = same-level neighbours with col < row (emitted by the row itself: bitwise equal to the
 * transposed entry); indeg[col] += 1 for every cross-level upper entry (integer atomics; indeg must be
 * zeroed).  Final CSR row = [indeg cross-level mirrors][samelow][rowcount own upper][diagonal]. */
int nksr_assemble_count(const nksr_hier_t* h, void* workspace, int32_t* rowcount, int32_t* crosscount, int32_t* samelow,
                        int32_t* indeg, void* stream);
/* Bytes of scratch (per-cell blocks + per-row column map) shared by nksr_assemble_count / nksr_assemble. */
size_t nksr_assemble_workspace_bytes(const nksr_hier_t* h);
/* Two-phase assembly of  sum_s w_s R_s^T R_s + reg I  (csrc/gram.hip, csrc/assemble.hip): per-cell dense blocks (fp32 MFMA),
 * then one wavefront per row.  rowptr = exclusive scan of (indeg + samelow + rowcount + 1), mir_off =
 * exclusive scan of crosscount.  Same-level lower, own upper entries and the diagonal are written straight
 * into cols_out / vals_out (tile-interleaved physical layout, see nksr_spmv_csr); the mirrored copies of the
 * cross-level entries go to mir_keys (src_row << col_bits | dst_row) / mir_vals.  Also writes diag_out and
 * b = sum_s w_s R_s^T t_s.
 * Levels >= 3 split: the block of a cell with R site rows is the sum, in order, of min(4^(d-2), 64, R / 128) parts.  With
 * split_scratch (nksr_assemble_split_bytes(h) bytes) a level of at most 65536 (cell, part) pairs whose tiles fit runs one wavefront
 * per pair and reduces in that order; otherwise (or NULL) one wavefront per cell walks its parts: the same bits either way. */
size_t nksr_assemble_split_bytes(const nksr_hier_t* h);
int nksr_assemble(const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, float reg, int col_bits,
                  void* workspace, const int32_t* rowptr, const int32_t* indeg, const int32_t* samelow,
                  const int32_t* mir_off, int col_format, int32_t* cols_out, float* vals_out, float* diag_out,
                  uint64_t* mir_keys, float* mir_vals, float* b_out, void* split_scratch, size_t split_scratch_bytes, void* stream);
/* Mirrors stably sorted by destination row (low col_bits of the key) -> their CSR slots;
 * mirptr = exclusive scan of indeg. */
int nksr_place_mirrors(const uint64_t* keys_sorted, const float* vals_sorted, int64_t n, int col_bits,
                       const int32_t* rowptr, const int32_t* mirptr, int col_format, int32_t* cols_out, float* vals_out,
                       void* stream);
/* The format-1 block of the coarse-level preconditioner (nksr_coarse_precond_t below) WITHOUT the fp32 CSR: word for word what
 * nksr_assemble (col_format 2) + nksr_place_mirrors + nksr_coarse_pack_count + nksr_coarse_pack give.  Four calls, two scans and one
 * keys-only sort between them (nksr_amd/fields/assembly.py: assemble_packed):
 *  1. nksr_assemble_packed: Gram blocks, then diag_out (every row's diagonal, ahead of the fill and bitwise the fill's), then the row
 *     fill with the drop test inside.  own_off = exclusive scan of (samelow + rowcount), mir_off = exclusive scan of crosscount,
 *     new_of_old = segment-major renumbering, local_col[r] = new_of_old[r] - seg_base[segment of r].  Kept own entries leave as final
 *     packed words inside [own_off[r], own_off[r + 1]) of own_out (lower run from its start, upper run from + samelow[r]); the mirror of
 *     every kept cross-level entry as  destination row (new) << 32 | half << 16 | local column of the source  inside
 *     [mir_off[r], mir_off[r + 1]) of mir_out; kept_out [3][n + 1] = kept lower / upper / mirror entries per row.
 *  2. nksr_packed_mirrors_compact: the kept mirror words as a dense list in ascending source row (kept_off = exclusive scan of
 *     kept_out[2]); it is then sorted stably on bits [32, 32 + bits(n)) (nksr_sort_keys_u64).
 *  3. nksr_packed_row_lengths: runs_out [2][n] = begin / end of every new row's run in the sorted list, lens_out [n] = run + kept own
 *     entries of new row i; packed_rowptr = exclusive scan of lens_out.
 *  4. nksr_packed_rows: row i = [mirrors][same-level lower][own upper], and dis_out (new order). */
int nksr_assemble_packed(const nksr_hier_t* h, const nksr_siteset_t* sets, int nsets, float reg, void* workspace,
                         const int32_t* samelow, const int32_t* mir_off, const int32_t* own_off, const int32_t* new_of_old,
                         const int32_t* local_col, float drop_tol, float* diag_out, uint32_t* own_out, uint64_t* mir_out,
                         int32_t* kept_out, void* split_scratch, size_t split_scratch_bytes, void* stream);
int nksr_packed_mirrors_compact(int32_t n, const uint64_t* mir_staged, const int32_t* mir_off, const int32_t* kept_mir,
                                const int32_t* kept_off, uint64_t* mir_dense, void* stream);
int nksr_packed_row_lengths(int32_t n, const uint64_t* mir_sorted, int64_t n_mir, const int32_t* kept, const int32_t* old_of_new,
                            int32_t* runs_out, int32_t* lens_out, void* stream);
int nksr_packed_rows(int32_t n, const uint64_t* mir_sorted, const int32_t* runs, const uint32_t* own, const int32_t* own_off,
                     const int32_t* samelow, const int32_t* kept, const int32_t* old_of_new, const int32_t* packed_rowptr,
                     const float* diag, uint32_t* packed_out, float* dis_out, void* stream);

/* ---- PCG (the CG SpMV is the roofline kernel) -------------------- */
/* nnz-chunked streaming CSR SpMV (csrc/spmv.hip).  cols/vals live in a tile-interleaved physical layout
 * chosen by col_format (the same value must be given to nksr_assemble / nksr_place_mirrors, which
 * write it):
 *   0: 256-entry tiles, logical entry m of a tile at 4*(m%64) + m/64, int32 columns, zero-padded (valid
 *      column 0, value 0) to a multiple of 4096 entries;
 *   1: 192-entry tiles, entry m at 3*(m%64) + m/64, padded to a multiple of 4608 entries; the SpMV reads
 *      the columns as one 64-bit word per three entries (21 bits each, nksr_pack_cols21 converts the
 *      int32 array written by the assembly): 6.67 instead of 8 bytes per entry, requires M <= 2^21.
 *   2 (nksr_assemble / nksr_place_mirrors only): plain CSR order, nnz entries, no padding -- the small coarse-level block of the
 *      preconditioner (nksr_coarse_precond_t); the streaming SpMV does not take it.
 * The plan (first row of every chunk) lives in `workspace` (nksr_spmv_workspace_bytes) and must be built
 * once per matrix with nksr_spmv_plan. */
size_t nksr_spmv_workspace_bytes(int64_t nnz);
int nksr_spmv_plan(const int32_t* rowptr, int32_t M, int64_t nnz, int col_format, void* workspace, void* stream);
int nksr_spmv_csr(const int32_t* rowptr, const void* cols, const float* vals, int32_t M, int64_t nnz, int col_format,
                  const float* x, float* y, void* workspace, void* stream);
/* int32 columns in the col_format-1 layout (n_padded entries, a multiple of 192) -> packed 64-bit words
 * (n_padded / 3 of them) */
int nksr_pack_cols21(const int32_t* cols32, int64_t n_padded, uint64_t* packed_out, void* stream);
/* Experimental kernel variants for tools/spmv_probe.py (0 = default). */
int nksr_spmv_set_variant(int v);
/* Scratch bytes required by nksr_pcg_solve. */
size_t nksr_pcg_workspace_bytes(int32_t M, int64_t nnz);
/* Jacobi-PCG, x0 = 0.  info_out (host, 3 doubles, may be NULL): [0]=iterations [1]=relative residual (negated on a hard failure:
 * r.z <= 0 with the Jacobi preconditioner, or NaN) [2]=segments whose coarse-level block lost definiteness (r.z <= 0) and that went on
 * with Jacobi alone from the current iterate (a restart on the device, no error).
 * Checks convergence every `check_every` iterations (one stream sync each) -- syncs.
 * coarse_precond (struct nksr_coarse_precond_t, declared below; NULL = Jacobi only): the diagonal block of the coarse levels. */
struct nksr_coarse_precond_s;
int nksr_pcg_solve(const int32_t* rowptr, const void* cols, const float* vals, const float* diag, int32_t M,
                   int64_t nnz, int col_format, const float* b, float* x, float tol, int max_iter, int check_every,
                   void* workspace, const struct nksr_coarse_precond_s* coarse_precond, double* info_out, void* stream);
/* Live profiling of the SpMV launches inside nksr_pcg_solve (HIP events on the solve's stream).
 * Returns and resets the accumulated milliseconds / launch count, then sets the enable flag. */
int nksr_pcg_profile(int enable, double* ms_out, int64_t* launches_out);
/* Durations (milliseconds) of the individual applications behind the totals the last nksr_pcg_profile call returned (host array,
 * at most `capacity` written); returns how many there were. */
int64_t nksr_pcg_profile_samples(float* ms_out, int64_t capacity);
/* Bytes of the launches timed since the last call (then reset): the algorithmic figure -- CSR: 8 nnz + 12 M + 4 per launch
 * (SURVEY.md section 8d); matrix-free operator: its algorithmic minimum, 4 bytes per stored entry + 4 per row and level (row ->
 * cell) + 116 per unknown (stencil, x, y) -- and the bytes the physical layout streams (col_format, padding, partial blocks). */
int nksr_pcg_profile_bytes(double* algorithmic_out, double* physical_out);
/* The launches of the last nksr_pcg_profile_bytes call priced by SURVEY.md section 8d's formula (equal to the algorithmic figure for
 * the CSR SpMV; 2 x 8 bytes per stored entry + 12 M + 4 for the matrix-free operator, more than it moves). */
double nksr_pcg_profile_survey_bytes(void);

/* ---- coarse-level block preconditioner of the PCG (csrc/cheb.hip) ----------------------------------------------------
 * The unknowns of the levels >= c0 (the LAST n of the M: unknowns are level-major) take `steps` Jacobi-preconditioned
 * Chebyshev steps on their diagonal block A_cc instead of one Jacobi step; all finer unknowns keep Jacobi.  A_cc: plain CSR
 * (nksr_assemble with col_format 2 on the hierarchy whose fine levels have n = 0, hcap = 0 and whose coarse levels are
 * re-based to offset 0), local indices.  lambda_max: largest eigenvalue of D^-1 A_cc (nksr_coarse_lambda_max, x ~1.1);
 * the polynomial targets the interval [lambda_max / ratio, lambda_max].
 * PRECONDITION on the plain block, relied on by every kernel that reads it and checked by none: every row holds at least its
 * diagonal entry, and holds it as its LAST entry (cols[rowptr[j + 1] - 1] == j, vals[rowptr[j + 1] - 1] == diag[j]); the entries
 * before it may come in any order.  The packer drops entry rowptr[j + 1] - 1 of every row unseen (the packed block has a unit
 * diagonal), and the Chebyshev step and the power iteration clamp their loads to that entry: an empty row would read entry -1. */
#define NKSR_PC_MAX_STEPS 16
/* Independent diagonal blocks of one system ("segments": the chunks of a batched chunk solve -- the reference solves its
 * chunks one after the other, examples/recons_by_chunk.py:26-29; here all chunks of a rank share every launch).  The unknowns
 * of segment c are the nranges index ranges [lo[c * nranges + k], hi[c * nranges + k]) (one per hierarchy level, possibly
 * empty).  The PCG gives every segment its own dot products (fixed, segment-relative reduction order), alpha / beta, stopping
 * test and iteration count: the iterates of a segment do not depend on which other segments share the launch.
 * NULL wherever a segments pointer is taken = one segment [0, M). */
typedef struct {
    int32_t nseg, nranges;
    const int32_t* lo;         /* [nseg * nranges] device */
    const int32_t* hi;         /* [nseg * nranges] device */
    double* info;              /* device [nseg * 2] or NULL: iterations, relative residual (negated when the segment stopped on
                                * r.z <= 0) of every segment, refreshed at every convergence check */
} nksr_segments_t;
typedef struct nksr_coarse_precond_s {
    int32_t first, n, steps, format;   /* format 0: plain CSR (rowptr / cols / vals / diag);  1: packed, see below */
    float lambda_scale, ratio; /* the eigenvalue bound of segment c is lambda_scale * lambda[c] (safety margin, ~1.1)          */
    const float* lambda;       /* device [nseg]: nksr_coarse_lambda_max; <= 0 / non-finite: that segment keeps plain Jacobi     */
    const int32_t* row_seg;    /* device [n]: segment of every coarse row; NULL with one segment                                */
    const int32_t* rowptr;     /* [n + 1] */
    const int32_t* cols;       /* [nnz_c] local column indices */
    const float* vals;         /* [nnz_c] */
    const float* diag;         /* [n] diagonal of A_cc */
    float* work;               /* [3 n] floats ([4 n] with format 1) */
    float* coef;               /* [nseg * (1 + 2 * NKSR_PC_MAX_STEPS)] floats: the solve writes the Chebyshev coefficients here */
    /* format 1 (nksr_coarse_pack): the Jacobi-scaled block S = D^-1/2 A_cc D^-1/2 without its unit diagonal, 4 bytes per entry --
     * (half-precision value << 16) | column local to the row's segment -- over the coarse unknowns renumbered segment-major; needs
     * < 2^16 coarse unknowns per segment.  row_seg is then in the NEW order.  The preconditioner stays a fixed symmetric positive
     * operator (all a CG preconditioner must be); a Chebyshev step streams half the bytes. */
    const uint32_t* packed;    /* [packed_rowptr[n]] */
    const int32_t* packed_rowptr; /* [n + 1] new order */
    const float* dis;          /* [n] D^-1/2, new order */
    const int32_t* old_of_new; /* [n] coarse row (PCG order) of every new row */
    const int32_t* seg_base;   /* [nseg + 1] first new row of every segment */
    const float* gersh;        /* device [nseg] or NULL: Gershgorin bound of the same spectrum (nksr_coarse_gershgorin); the interval's upper
                                * end is min(lambda_scale * lambda[c], gersh[c]) */
} nksr_coarse_precond_t;
/* Gershgorin bound per segment of the Jacobi-scaled block described by pc (either format; work: n floats): gersh_out [nseg]. */
int nksr_coarse_gershgorin(const nksr_coarse_precond_t* pc, int32_t nseg, float* work, float* gersh_out, void* stream);
/* format-1 block from the plain CSR: new_of_old / old_of_new = the segment-major renumbering, row_seg_new / seg_base in the new
 * order, packed_rowptr = exclusive sum of the kept entries per row (nksr_coarse_pack_count) in the new order.  Off-diagonal entries
 * with |S_ij| < drop_tol are left out (0 keeps all; S_ij = S_ji bitwise, so the block stays symmetric).  Writes packed_out, dis_out. */
int nksr_coarse_pack_count(const int32_t* rowptr, const int32_t* cols, const float* vals, const float* diag, int32_t n,
                           const int32_t* old_of_new, float drop_tol, int32_t* lens_out, void* stream);
int nksr_coarse_pack(const int32_t* rowptr, const int32_t* cols, const float* vals, const float* diag, int32_t n,
                     const int32_t* old_of_new, const int32_t* new_of_old, const int32_t* row_seg_new, const int32_t* seg_base,
                     const int32_t* packed_rowptr, float drop_tol, uint32_t* packed_out, float* dis_out, void* stream);
/* eigenvalue bounds of a format-1 block (power iteration on S, work: 2 n floats): lambda_out [nseg] */
int nksr_coarse_lambda_max_packed(const nksr_coarse_precond_t* pc, int32_t nseg, int iters, float* work, float* lambda_out, void* stream);
/* power iteration (iters steps from the all-ones vector, work: 2 n floats): lambda_out (device, [nseg]) = ||v_k|| / ||v_{k-1}||
 * over the coarse rows of every segment (`first` = unknown index of coarse row 0; the ranges below it are skipped). */
int nksr_coarse_lambda_max(const int32_t* rowptr, const int32_t* cols, const float* vals, const float* diag, int32_t n, int iters,
                           float* work, float* lambda_out, const nksr_segments_t* segments, int32_t first, void* stream);
/* The preconditioner by itself, exactly as nksr_pcg_solve applies it: z = p(A_cc) r for the coarse slices r, z (device, [pc->n], PCG
 * order; pc->first is not used).  Validates pc as the solve does (1 .. NKSR_PC_MAX_STEPS steps, lambda_scale > 0, ratio > 1, the
 * arrays of its format), writes the coefficient table of the nseg segments into pc->coef from pc->lambda / pc->gersh, then runs
 * the `steps` Chebyshev steps in pc->work.  Asynchronous on `stream`. */
int nksr_coarse_precond_apply(const nksr_coarse_precond_t* pc, int32_t nseg, const float* r, float* z, void* stream);

/* ---- matrix-free ("fused") operator and solve: reconstruct(..., fused_mode=True), examples/recons_waymo.py:33,
 *      recons_waymo_cpu.py:58, gis_app.py:40; KernelField.solve (csrc/fused_tables.hip: the tables, csrc/fused_sweep.hip: the pass over the rows, csrc/fused.hip:
 *      the second product, these entry points and the solve).  The system matrix is never built:
 *      y = (sum_s R_s^T R_s + reg I) x is applied from the dense-slot kernel rows, cell by cell. ------------------ */
typedef struct {
    int32_t depth, M, n_multi, n_big;
    int64_t rows_total;        /* rows of all site sets in ONE Morton-ordered list (level-0 key of the site; position rows 1 per site,
                                * gradient rows 3 per site); also the level stride of rows_all / row_cells                   */
    const float* rows_all;     /* LEVEL-MAJOR dense-slot rows [depth][rows_total][27], pre-multiplied by sqrt(w) (nksr_kernel_rows, level_stride, row_index) */
    const float* targets_all;  /* [rows_total] right-hand side values pre-multiplied by sqrt(w) (0 for rows without a target); may be NULL if unused */
    const int32_t* row_cells;  /* [depth][rows_total] GLOBAL unknown index of the row's level-d cell, -1 = none (nksr_kernel_rows) */
    const int32_t* nbr32;      /* [M, 32]: [0..26] GLOBAL unknown index of every neighbour voxel or -1; [27] block base, [28] / [29] first / last row of
                                * the cell, [30] / [31] unused (0) (nksr_fused_tables) */
    const int32_t* nbrT;       /* [27, M]: the same neighbour indices SLOT-MAJOR (the second product's gather runs one lane per unknown) */
    const int32_t* item_begin; /* [nksr_fused_item_entries(rows_total)] first row of every work item of the sweep (nksr_fused_block_counts) */
    const int32_t* offsets;    /* [M + 1] partial blocks of a cell = [offsets[j], offsets[j + 1])                             */
    const int32_t* multi;      /* [n_multi] the cells with partial blocks (cells whose rows span several 256-row workgroups of the sweep):
                                * first the n_big cells with more than 16 blocks (one workgroup each in the per-cell sum), then the others */
    int64_t nblocks;           /* offsets[M]                                                                                 */
    uint64_t* nnz_counter;     /* device array of nksr_fused_count_words(rows_total) words or NULL: nksr_fused_rhs_diag leaves the non-zero
                                * slots of rows_all in word 0 = the stored entries of G and Q (roofline accounting).
                                * Words 1 .. are scratch without an initial value: one count per workgroup of the sweep (plain
                                * stores), added into word 0 afterwards -- the sweep shares no word between its workgroups */
    void* workspace;           /* nksr_fused_workspace_bytes(nblocks, M)                                                     */
    float* cell_sums;          /* [27, M] per-cell block sums, slot-major, ZERO-INITIALISED by the caller (cells without rows are never written) */
    const int32_t* item_seg;   /* batched chunks (nksr_segments_t), both or neither: [ceil(rows_total / 32) + 1] segment of every 32-row window
                                * of the row list (a segment's rows are padded to a multiple of 256) and                      */
    const int32_t* unknown_seg;/* [M] segment of every unknown: the solve skips the rows / unknowns of segments that have converged */
    /* FACTOR FORM (kernel_dim 4; nksr_kernel_factors): fac_vec != NULL replaces rows_all (which may then be NULL) -- the sweep rebuilds the
     * 27 slots of every row in registers from 16-byte records and the psi stencil of the row's cell.  A normal site owns FOUR rows
     * of the list (header + one per axis); the header row is all-zero. */
    const float* fac_vec;      /* [depth][rows_total][4] phi (position / header rows) or d phi / d x_a (gradient rows), times sqrt(w); 16-byte aligned */
    const float* fac_pos;      /* [rows_total][4] x * inv_w0 (3 floats) + the row's kind as int bits: 0 position, 1 header, 2 + a gradient row of axis a */
    const float* psi_all;      /* [M][4] psi of every unknown, levels concatenated (nksr_voxel_psi)                              */
    float inv_w0;              /* 1 / finest voxel size (fp32, as in nksr_hier_t)                                               */
    int32_t dense_from;        /* nksr_fused_rhs_diag / nksr_fused_expand_rows: the rebuilt rows of the levels >= dense_from are also written to */
    float* dense_out;          /* [depth - dense_from][rows_total][27] (NULL: not wanted) -- what the coarse-level block of the preconditioner is assembled from */
} nksr_fused_op_t;
/* A UNIT is a maximal run of rows that lie in the same cell at every level (the rows of one level-0 cell); work item i of the sweep =
 * the units that start in the 32-row window [32 i, 32 i + 32) = rows [item_begin[i], item_begin[i + 1]); eight items are a workgroup.
 * A cell whose rows lie inside one workgroup is finished by the sweep, a cell whose rows reach into k > 1 workgroups owns k partial
 * blocks.  rows_all / targets_all must be readable 320 rows past rows_total (unconditional loads).
 * nksr_fused_block_counts: span_out [3, M] (first / last row of every cell, -1 = none; first workgroup), item_begin_out [nksr_fused_item_entries],
 * counts_out [M + 1] (0 or k; last entry 0) -> exclusive scan = offsets -> nksr_fused_tables (nbr32_out [M, 32], nbrT_out [27, M]). */
int64_t nksr_fused_item_entries(int64_t rows_total);
int64_t nksr_fused_count_words(int64_t rows_total);   /* words of nksr_fused_op_t.nnz_counter: the total + one per workgroup of the sweep */
int nksr_fused_block_counts(int32_t depth, int32_t M, int64_t rows_total, const int32_t* row_cells, int32_t* span_out, int32_t* item_begin_out,
                            int32_t* counts_out, void* stream);
int nksr_fused_tables(const nksr_hier_t* h, int64_t rows_total, const int32_t* item_begin, const int32_t* offsets, const int32_t* span,
                      int32_t* nbr32_out, int32_t* nbrT_out, void* stream);
size_t nksr_fused_workspace_bytes(int64_t nblocks, int32_t M);
/* b = sum_s R_s^T t_s and diag = reg + sum_s diag(R_s^T R_s) (either may be NULL): one sweep over the rows serves both. */
int nksr_fused_rhs_diag(const nksr_fused_op_t* op, float reg, float* b_out, float* diag_out, void* stream);
/* Factor form only: the rebuilt rows of the levels >= op->dense_from written dense into op->dense_out (one more set-up sweep;
 * nksr_fused_rhs_diag does the same on its way when dense_out is set).  Scratch: the operator's workspace and cell_sums. */
int nksr_fused_expand_rows(const nksr_fused_op_t* op, void* stream);
/* y = (sum_s R_s^T R_s + reg I) x */
int nksr_fused_apply(const nksr_fused_op_t* op, float reg, const float* x, float* y, void* stream);
/* Jacobi-PCG with that operator; pcg_workspace: nksr_pcg_vector_workspace_bytes(M), or ..._seg(M, nseg, nranges) with segments.
 * Syncs like nksr_pcg_solve.  info_out (3 doubles): [0] = iterations (max over the segments), [1] = relative residual (max; negated if a
 * segment failed hard), [2] = segments that fell back to Jacobi (see nksr_pcg_solve). */
size_t nksr_pcg_vector_workspace_bytes(int32_t M);
size_t nksr_pcg_vector_workspace_bytes_seg(int32_t M, int32_t nseg, int32_t nranges);
int nksr_pcg_solve_fused(const nksr_fused_op_t* op, float reg, const float* diag, const float* b, float* x, float tol, int max_iter,
                         int check_every, void* pcg_workspace, const nksr_coarse_precond_t* coarse_precond /* or NULL: Jacobi */,
                         const nksr_segments_t* segments /* or NULL */, double* info_out, void* stream);

/* ---- chunk plumbing of reconstruct(chunk_size=...) (csrc/chunks.hip; examples/recons_by_chunk.py:29) ---------------------------
 * The chunk grid: chunk id = (cx * grid[1] + cy) * grid[2] + cz; along a split axis (grid[a] > 1) chunk j has the core [lo_j, hi_j),
 * solves the points with  lo_sel[a][j] <= x < hi_sel[a][j]  (= fp32(lo_j - band), fp32(hi_j + band)) and weighs
 * w = prod_a clamp((x - lo_w[a][j]) * inv_2ov, 0, 1) * clamp((hi_w[a][j] - x) * inv_2ov, 0, 1)  (lo_w = fp32(lo_j - ov), hi_w = fp32(hi_j + ov),
 * factors multiplied in the order up_x, dn_x, up_y, ...; an axis that is not split contributes nothing).  Candidates of a point: the
 * chunks within `reach` of its home chunk floor((x - origin) * inv_cs). */
typedef struct {
    int32_t grid[3];
    int32_t reach;
    float origin[3];
    float inv_cs, inv_2ov;
    const float* lo_sel[3];    /* device, [grid[a]] each; may be NULL for an axis that is not split */
    const float* hi_sel[3];
    const float* lo_w[3];
    const float* hi_w[3];
    const float* shift;        /* device [nchunk, 3]: translation of every chunk into its slot of the exploded frame (mode 1) */
} nksr_chunk_grid_t;
/* mode 0: (point, chunk) pairs of the solve's input; mode 1: pairs with a positive blend weight.  chunk_flag [nchunk] >= 0: the chunk
 * takes part.  Count pass -> exclusive scan (offsets, n + 1 entries) -> fill pass: pairs of a point in ascending chunk order;
 * mode 1 also writes the weight and the translated position x + shift[chunk] (one fp32 rounding). */
int nksr_chunk_pair_counts(const nksr_chunk_grid_t* grid, int mode, const float* xyz, int64_t n, const int32_t* chunk_flag,
                           int32_t* counts_out, void* stream);
int nksr_chunk_pair_fill(const nksr_chunk_grid_t* grid, int mode, const float* xyz, int64_t n, const int32_t* chunk_flag,
                         const int32_t* offsets, int64_t* pair_point_out, int32_t* pair_chunk_out, float* pair_w_out,
                         float* pair_xyz_out, void* stream);
/* f = sum_k w_k f_k / max(sum_k w_k, 1e-20) over the pairs [offsets[i], offsets[i + 1]) of query i, in that order (+ the same for the
 * gradient when pair_grad / grad_out are given). */
int nksr_chunk_blend(int64_t n, const int32_t* offsets, const float* pair_w, const float* pair_f, const float* pair_grad,
                     float* f_out, float* grad_out, void* stream);
/* Seam candidates of a rank's mesh piece (the merge on rank 0, nksr_amd/dist.py): vertex i lies on the lattice edge (vertex vkey[i],
 * axis[i]); flag = 1 when one of the four lattice cells around that edge belongs to another rank -- owner[chunk of the centre of the
 * cell's base voxel] != rank, base voxel = floor(cell / cells_per_voxel), centre = (base + 0.5) w0, chunk as nksr_chunk_pair_counts. */
int nksr_edge_seam_flags(const nksr_chunk_grid_t* grid, const int64_t* vkey, const int8_t* axis, int64_t n, int32_t cells_per_voxel, float w0,
                         const int32_t* owner, int32_t rank, uint8_t* flags_out, void* stream);
/* Which points lie in a core this rank owns (reach = 0) or within `reach` of one along the split axes: flag = 1 when
 * owner[chunk of (x + o)] == rank for an offset o in {-reach, 0, +reach} per split axis (the cells a rank meshes / evaluates). */
int nksr_points_owner_flags(const nksr_chunk_grid_t* grid, const float* xyz, int64_t n, float reach, const int32_t* owner, int32_t rank,
                            uint8_t* flags_out, void* stream);
/* Halo selection of a batch of chunks, one level (the payload of the rank exchange; chunking.pack_halos):
 * voxel i (keys ascending) belongs to chunk seg = the last of the ascending key ranges klo [nchunk] that starts at or before its key;
 * flag = 1 when its centre (ijk + 0.5) w - shift[seg] lies in one of the chunk's band intervals [tlo, thi] ([nchunk, 3, 2] each, an
 * unused interval = (+inf, -inf)) along some axis. */
int nksr_halo_band_flags(const int64_t* keys, const int32_t* ijk, int64_t n, const int64_t* klo, int32_t nchunk, const float* shift,
                         const float* tlo, const float* thi, float w, int32_t* seg_out, int32_t* flags_out, void* stream);

/* ---- grid-hash nearest neighbours (csrc/knn_normals.hip, knn_sdf.hip, knn_query.hip) ----------------------------------------------------
 * Points Morton-sorted by a uniform grid of size `cell` (keys from nksr_point_keys with inv_w0 =
 * inv_cell); start/end = nksr_site_ranges of the occupied cells; hkeys/hvals = their hash. */
/* kNN-PCA normals (unoriented): nksr.get_estimate_normal_preprocess_fn, examples/recons_waymo.py:36,
 * recipe examples/recons_waymo_cpu.py:21-41.  valid_out[i]=0 where fewer than k points lie within
 * max_ring cells. */
int nksr_knn_pca_normals(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end,
                         const int64_t* hkeys, const int32_t* hvals, int32_t hcap, float cell, float inv_cell, int k,
                         int max_ring, float* normal_out, float* radius2_out, int32_t* valid_out,
                         int32_t* todo_work /* [n] ints: one wavefront per query (candidates through LDS); NULL: one thread per query */,
                         void* stream);
/* An octree over ONE Morton-sorted cloud (ext.sdfgen, reference ext/common/kdtree_cuda.cu: the role of its kd-tree): level l has cells
 * of size cell * 2^l, its cell keys are the level-0 keys >> 3 l (sorted unique); start / end = the point range of every cell, hkeys /
 * hvals / hcap the key -> cell hash of the level, and for l > 0 child [n_l + 1] / cmask [n_l] = the range of a cell's children on level
 * l - 1 and their occupied octants (nksr_knn_pyramid_level builds start / end / child / cmask of a level from the level below).
 * nksr_sdf_from_points_pyramid / nksr_knn_mean_dist_pyramid = the nb_points <= 32 path of nksr_sdf_from_points / nksr_knn_mean_dist
 * at every scale, EVERY level in one launch: a query climbs to the first level with a point within one cell of it and takes its k
 * nearest there (kept sorted in registers; cells nearest first, descended with box pruning down to cells of <= leaf points), climbing on
 * only when fewer than k lie within max_ring rings; valid = 0: not even the coarsest level holds k points in reach.  levels = 1 (no
 * child / cmask) is a single grid: what the host retries such rows on, with a coarser cell. */
#define NKSR_KNN_LEVELS 12
typedef struct {
    const float* xyz_sorted;
    const int32_t* start[NKSR_KNN_LEVELS];
    const int32_t* end[NKSR_KNN_LEVELS];
    const int32_t* child[NKSR_KNN_LEVELS];
    const uint8_t* cmask[NKSR_KNN_LEVELS];
    const int64_t* hkeys[NKSR_KNN_LEVELS];
    const int32_t* hvals[NKSR_KNN_LEVELS];
    int32_t hcap[NKSR_KNN_LEVELS];
    int32_t levels, leaf;
    float cell, inv_cell;
} nksr_knn_pyramid_t;
int nksr_knn_pyramid_level(const int64_t* child_keys, int32_t n_child, const int32_t* child_start, const int32_t* child_end,
                           const int64_t* keys, int32_t n, int32_t* child_out, uint8_t* cmask_out, int32_t* start_out, int32_t* end_out,
                           void* stream);
int nksr_sdf_from_points_pyramid(const nksr_knn_pyramid_t* pyramid, const float* normal_sorted, const float* ref_std_sorted, const float* query,
                                 int64_t nq, int k, int max_ring, float stdv, int imls, float* sdf_out, float* grad_out, int32_t* valid_out,
                                 void* stream);
int nksr_knn_mean_dist_pyramid(const nksr_knn_pyramid_t* pyramid, int64_t n, int k, int max_ring, float* out, int32_t* valid_out, void* stream);
/* Signed distance of arbitrary queries to an oriented cloud from their k = nb_points nearest reference points: the training
 * ground truth ext.sdfgen.sdf_from_points(queries, ref_xyz, ref_normal, nb_points, stdv, compute_grad, imls, adaptive_knn)
 * (ext/sdfgen/sdf_from_points.cu:32-235; models/loss.py:85, dataset/av_gt_geometry.py:72).  imls = 0: nearest-neighbour magnitude
 * (|n.(x-p)| inside stdv * ref_std[p], |x-p| outside) with the sign voted by the k neighbours; imls != 0: IMLS weights
 * exp(-|x-p_k|^2 / stdv^2).  ref_std_sorted may be NULL (= 1); grad_out may be NULL.  valid_out[i] = 0: fewer than k points within
 * max_ring cells (retry on a coarser grid).  nksr_knn_mean_dist: mean distance of every reference point to its k nearest
 * (itself included) = ref_std for adaptive_knn = k.  These two are the ANY-k path: one grid, the k-th distance found by bisection
 * (~35 scans of the candidate block per query); the host sends them nb_points > 32 only. */
int nksr_sdf_from_points(const float* xyz_sorted, const float* normal_sorted, const float* ref_std_sorted, const int32_t* start,
                         const int32_t* end, const int64_t* hkeys, const int32_t* hvals, int32_t hcap, float cell, float inv_cell,
                         const float* query, int64_t nq, int k, int max_ring, float stdv, int imls, float* sdf_out, float* grad_out,
                         int32_t* valid_out, void* stream);
int nksr_knn_mean_dist(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                       const int32_t* hvals, int32_t hcap, float cell, float inv_cell, int k, int max_ring, float* out,
                       int32_t* valid_out, void* stream);
/* index (into the sorted cloud) of the nearest point of every query: fields.PCNNField,
 * examples/recons_colored_mesh.py:28 */
int nksr_nearest_index(const float* xyz_sorted, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                       const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const float* query, int64_t nq,
                       int max_ring, int32_t* index_out, void* stream);
/* The k nearest reference points of arbitrary queries WRITTEN OUT (nksr_amd/cloud.py CloudIndex.knn), 1 <= k <= 32: idx_out [nq, k]
 * = indices into the sorted cloud, dist2_out [nq, k] = their squared fp32 distances, ascending; valid_out [nq] = 0 where the search
 * did not reach k points (that row is left untouched: retry on a coarser grid).  query NULL: the queries are the first nq points of
 * the sorted cloud itself (nq <= n_ref).  exclude_self != 0: ONE reference point is left out of every row -- the one whose sorted
 * index is self_index[i], or i itself when self_index is NULL; other points at the same position are kept (k + 1 <= n_ref).
 * The search is that of nksr_sdf_from_points_pyramid. */
int nksr_knn_query_pyramid(const nksr_knn_pyramid_t* pyramid, int64_t n_ref, const float* query, int64_t nq, int k, int exclude_self,
                           const int32_t* self_index, int max_ring, int32_t* idx_out, float* dist2_out, int32_t* valid_out, void* stream);
/* count_out [nq] = number of reference points with |x - q|^2 <= radius^2 (fp32, the rounding sequence of the kNN kernels) among the
 * 27 cells around the query: the grid must have cell >= radius.  cap > 0: the scan of a query stops once its count reaches cap and
 * min(count, cap) is returned; cap <= 0: no limit.  query / exclude_self / self_index as above.  Integers only, no atomics. */
int nksr_radius_count(const float* xyz_sorted, int64_t n_ref, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                      const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const float* query, int64_t nq, float radius,
                      int32_t cap, int exclude_self, const int32_t* self_index, int32_t* count_out, void* stream);

/* ---- rigid registration: one ICP pass (csrc/register.hip; nksr_amd/register.py: cloud.icp) -----------------------------------
 * nksr_icp_accumulate: one lane per source point s (fp32 [n_src, 3]).  p = R s + t in fp64, transform [12] (device) = the upper three
 * rows of the 4 x 4 matrix, row-major: p_a = ((T[4a] s_x + T[4a+1] s_y) + T[4a+2] s_z) + T[4a+3], every product and sum rounded on its
 * own (no fused multiply-add, here and in every term below: the terms are the ones plain fp64 arithmetic gives).  p32 = fl32(p)
 * serves the search only: the nearest point q of the grid (arguments as nksr_radius_count takes them; cell >= radius) among the 27
 * cells around p32 with knn_d2(p32 - q) <= fl32(radius)^2; on an exact tie the point with the smallest perm [n_ref] (int64: the grid's
 * order -> the caller's).  A p32 that is not finite or has |p32| * inv_cell >= 2^20 - 8 on an axis has no correspondence.
 * corr_out [n_src] (int64) = perm of that point, or -1.  partials_out [ceil(n_src / NKSR_ICP_BLOCK), NKSR_ICP_FIELDS] = per workgroup
 * the fp64 sums over its points with a correspondence, reduced in a fixed order (wavefront butterfly, then the waves in order; no
 * atomics), with d = p - q, p' = p - c, q' = q - c, c = centre [3] (device), |d|^2 = (d_x d_x + d_y d_y) + d_z d_z:
 *   both methods   [NKSR_ICP_COUNT] the count, [NKSR_ICP_D2] sum |d|^2
 *   method 0 (point)  [NKSR_ICP_PT_P + a] sum p'_a, [NKSR_ICP_PT_Q + a] sum q'_a, [NKSR_ICP_PT_PQ + 3 a + b] sum p'_a q'_b
 *   method 1 (plane, normal_sorted [n_ref, 3] = the normals n in the grid's order): r = (n_x d_x + n_y d_y) + n_z d_z,
 *     J = (p' x n, n) with (p' x n)_x = p'_y n_z - p'_z n_y (cyclic); [NKSR_ICP_PL_JJ + k] sum J_a J_b over a <= b, row after row
 *     (k = 0 .. 20), [NKSR_ICP_PL_JR + a] sum J_a r, [NKSR_ICP_PL_RR] sum r^2
 * and zeros in the fields a method does not use.  n_src == 0: nothing is touched.
 * nksr_icp_reduce: sums_out [NKSR_ICP_FIELDS] = the column sums of partials [nrows, NKSR_ICP_FIELDS], one workgroup, fixed order. */
#define NKSR_ICP_BLOCK 256
#define NKSR_ICP_FIELDS 32
#define NKSR_ICP_COUNT 0
#define NKSR_ICP_D2 1
#define NKSR_ICP_PT_P 2
#define NKSR_ICP_PT_Q 5
#define NKSR_ICP_PT_PQ 8
#define NKSR_ICP_PL_JJ 2
#define NKSR_ICP_PL_JR 23
#define NKSR_ICP_PL_RR 29
int nksr_icp_accumulate(const float* xyz_sorted, int64_t n_ref, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                        const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const int64_t* perm, const float* normal_sorted,
                        const float* source, int64_t n_src, const double* transform, const double* centre, float radius, int method,
                        int64_t* corr_out, double* partials_out, void* stream);
int nksr_icp_reduce(const double* partials, int64_t nrows, double* sums_out, void* stream);

/* ---- point-cloud segmentation (csrc/segment.hip; nksr_amd/segment.py: cloud.cluster_dbscan, cloud.segment_plane) ----------------
 * DBSCAN on a grid as nksr_radius_count takes it (cell >= radius; n < 2^31 points in the grid's order).  j is a neighbour of i iff
 * knn_d2(x_j - x_i) <= fl32(radius)^2, the predicate of nksr_radius_count; core [n] (uint8) = the points with at least min_points
 * neighbours, themselves included: (nksr_radius_count(cap = min_points, exclude_self = 0) >= min_points).
 * nksr_dbscan_components: union-find over the pairs of core points that are neighbours.  parent_out [n] = the smallest sorted index of
 *   the point's component (-1 for a point that is not core), root_flags_out [n + 1] = (parent_out[i] == i), then a 0.
 * nksr_dbscan_min_caller: min_index_out [n]: at every root r the smallest perm [n] (int64: the grid's order -> the caller's) over the
 *   points with parent[i] == r; 0x7F7F7F7F elsewhere.  Integer atomicMin: independent of the order the lanes run in.
 * nksr_dbscan_border: label [n] holds the labels of the core points on entry (anything at the others); on return every point that is
 *   not core holds the smallest label among the core points that are its neighbours, or -1 without one.
 * Plane RANSAC.  xyz [n, 3] fp32 in the caller's order; a plane is (a, b, c, d) in fp64; the residual of a point is
 * s = ((a x + b y) + c z) + d in fp64 with every product and sum rounded on its own; inlier iff |s| <= threshold (finite, >= 0).
 * nksr_plane_score: counts_out [n_planes] (int32) = the inliers of every plane of planes [n_planes, 4] (device); -1 for a plane that
 *   is not finite or has a = b = c = 0.  Integer atomics only.
 * nksr_plane_moments: plane [4], centre [3] (device).  mask_out [n] (uint8) = inlier; partials_out [ceil(n / NKSR_ICP_BLOCK),
 *   NKSR_ICP_FIELDS] = per workgroup the fp64 sums over its inliers, x' = x - centre: [NKSR_PLANE_COUNT] the count, [NKSR_PLANE_SUM + a]
 *   sum x'_a, [NKSR_PLANE_MOMENT + k] sum x'_a x'_b over a <= b, row after row (xx, xy, xz, yy, yz, zz), zeros behind; fixed order, no
 *   atomics: the rows go to nksr_icp_reduce. */
#define NKSR_PLANE_COUNT 0
#define NKSR_PLANE_SUM 1
#define NKSR_PLANE_MOMENT 4
#define NKSR_PLANE_FIELDS 10
int nksr_dbscan_components(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                           const int32_t* hvals, int32_t hcap, float cell, float inv_cell, float radius, const uint8_t* core,
                           int32_t* parent_out, int32_t* root_flags_out, void* stream);
int nksr_dbscan_min_caller(const int32_t* parent, const int64_t* perm, int64_t n, int32_t* min_index_out, void* stream);
int nksr_dbscan_border(const float* xyz_sorted, int64_t n, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                       const int32_t* hvals, int32_t hcap, float cell, float inv_cell, float radius, const uint8_t* core, int32_t* label,
                       void* stream);
int nksr_plane_score(const float* xyz, int64_t n, const double* planes, int64_t n_planes, double threshold, int32_t* counts_out,
                     void* stream);
int nksr_plane_moments(const float* xyz, int64_t n, const double* plane, const double* centre, double threshold, uint8_t* mask_out,
                       double* partials_out, void* stream);

/* ---- global registration (csrc/fpfh.hip, csrc/global_register.hip; nksr_amd/global_register.py: cloud.compute_fpfh_feature,
 * cloud.match_features, cloud.registration_ransac_based_on_feature_matching) ------------------------------------------------------
 * Fast Point Feature Histograms.  xyz / normal [n, 3] fp32 in ONE order (normals of unit length), idx [n, k] (int32, indices into that
 * order) and d2 [n, k] (fp32) = the k neighbours of every point and their squared distances, 1 <= k <= NKSR_FPFH_MAX_K.  Neighbour m
 * of point i, j = idx[i, m], TAKES PART iff d2[i, m] <= fl32(radius)^2 (the fp32 product), d2[i, m] > 0 and the cross product v below
 * is not (0, 0, 0).  Pair features: fp64 from the fp32 inputs widened, every product and sum rounded on its own (no fused
 * multiply-add), a dot product a.b = (a_x b_x + a_y b_y) + a_z b_z, a cross product (a x b)_x = a_y b_z - a_z b_y (cyclic):
 *   d = x_j - x_i, L = sqrt(d.d), a1 = (n_i.d) / L, a2 = (n_j.d) / L
 *   |a1| < |a2|:  u = n_j, o = n_i, d <- -d, f2 = -a2;     otherwise:  u = n_i, o = n_j, f2 = a1
 *   v = d x u, |v| = sqrt(v.v), v <- v / |v| per component;  w = u x v;  f1 = v.o;  f0 = atan2(w.o, u.o)
 *   b0 = floor((11 (f0 + pi)) / (2 pi)), b1 = floor((11 (f1 + 1)) / 2), b2 = floor((11 (f2 + 1)) / 2), each clamped to 0 .. 10
 * nksr_spfh: count_out [n, NKSR_FPFH_BINS] (int32) = per point the number of its participating neighbours in bins b0, 11 + b1 and
 *   22 + b2; n_out [n] (int32) = their number; mask_out [n] (uint32) = bit m set iff neighbour m takes part.  Integers only, no
 *   atomics.  n == 0: nothing is touched.
 * nksr_fpfh: out [n, NKSR_FPFH_BINS] (fp32) from count / n_nb / mask as nksr_spfh wrote them, all fp64 in this order:
 *   S[i, b] = (double) count[i, b] * (100 / (double) n_nb[i]), 0 where n_nb[i] = 0;
 *   F[i, b] = sum over the set bits m of mask[i], ascending, one after another: S[idx[i, m], b] / (double) d2[i, m];
 *   per third g = 0, 1, 2: s_g = the sum of F[i, 11 g .. 11 g + 10] in ascending b; s_g > 0: F[i, b] <- F[i, b] * (100 / s_g);
 *   out[i, b] = fl32(F[i, b] + S[i, b]).  Fixed order, no atomics: the same call gives the same bits.
 * nksr_feature_match: for every row a of A [na, NKSR_FPFH_BINS] (fp32) the row b of B [nb, NKSR_FPFH_BINS] with the smallest
 *   D = sum_j (A[a, j] - B[b, j])^2, accumulated in fp32 in ascending j (difference, product, sum, each rounded on its own; no
 *   expansion of the square), the lowest b among equal D.  idx_out [na] (int32) = b, dist2_out [na] = D; a row of A for which no b
 *   gives a finite D (a NaN or an infinity in it, or nb == 0) has idx -1 and dist2 +inf.  keys_work [na] (uint64) is scratch: the
 *   rows of B are split over workgroups whose partial answers meet in one integer atomicMin on (bits of D) << 32 | b -- D >= 0, so
 *   its bits order as an integer; no floating-point atomics.  na == 0: nothing is touched.  na, nb < 2^31.
 * nksr_pose_score: pairs (p, q) = (src [n_pairs, 3], tgt [n_pairs, 3]) fp32; transforms [n_hyp, 12] (fp64, device) = the upper three
 *   rows of 4 x 4 matrices, row-major.  p' = R p + t as nksr_icp_accumulate states it, e = p' - q, inlier iff
 *   (e_x e_x + e_y e_y) + e_z e_z <= threshold * threshold (fp64, no fused multiply-add).  counts_out [n_hyp] (int32) = the inliers
 *   of every transform, -1 for one with an entry that is not finite.  Integer atomics only.  n_hyp <= NKSR_POSE_MAX_H.
 * nksr_corr_accumulate: the rows of nksr_icp_accumulate's method 0 (NKSR_ICP_COUNT, NKSR_ICP_D2, NKSR_ICP_PT_P, _Q, _PQ; zeros
 *   behind) over the inliers -- the test above -- of ONE transform [12] among given pairs, about centre [3] (both device):
 *   partials_out [ceil(n_pairs / NKSR_ICP_BLOCK), NKSR_ICP_FIELDS], the same fixed order (the rows go to nksr_icp_reduce);
 *   mask_out [n_pairs] (uint8) = inlier.  n_pairs == 0: nothing is touched. */
#define NKSR_FPFH_BINS 33
#define NKSR_FPFH_MAX_K 32
#define NKSR_POSE_MAX_H (1 << 20)
int nksr_spfh(const float* xyz, const float* normal, int64_t n, const int32_t* idx, const float* d2, int k, float radius,
              int32_t* count_out, int32_t* n_out, uint32_t* mask_out, void* stream);
int nksr_fpfh(const int32_t* count, const int32_t* n_nb, const uint32_t* mask, int64_t n, const int32_t* idx, const float* d2, int k,
              float* out, void* stream);
int nksr_feature_match(const float* A, int64_t na, const float* B, int64_t nb, uint64_t* keys_work, int32_t* idx_out, float* dist2_out,
                       void* stream);
int nksr_pose_score(const float* src, const float* tgt, int64_t n_pairs, const double* transforms, int64_t n_hyp, double threshold,
                    int32_t* counts_out, void* stream);
int nksr_corr_accumulate(const float* src, const float* tgt, int64_t n_pairs, const double* transform, const double* centre,
                         double threshold, uint8_t* mask_out, double* partials_out, void* stream);

/* ---- voxel reduction of a point cloud (csrc/cloud.hip; nksr_amd/cloud.py voxel_downsample) -----------------------------------
 * order [n] = point indices sorted by voxel key, start / end [n_vox] = the run of every voxel in it (nksr_run_table_u64 of the sorted
 * keys: start_out without its last entry, and without its first). mean_xyz_out [n_vox, 3] and mean_attr_out [n_vox, C] = the mean of xyz [n, 3] and of attr [n, C] (C = 0: attr and
 * mean_attr_out NULL; C <= NKSR_VOXEL_REDUCE_MAX_C) over every run, count_out [n_vox] its length.  Sums are fp64 in an order fixed by
 * (n_vox, start, end, group) alone -- a wavefront owns `group` consecutive voxels and walks their sorted positions 64 at a time, a
 * segmented tree inside the 64, tile after tile -- divided in fp64 and rounded once to fp32: no atomics, every run repeats bit for
 * bit.  group: voxels per wavefront, 1 .. 64, 0 = chosen from n_vox.  nearest_out [n_vox] (may be NULL) = the sorted position of the
 * run's point nearest the (fp64) mean, the lowest position on a tie.  An index of `order` outside [0, n) is left out of sum and count. */
#define NKSR_VOXEL_REDUCE_MAX_C 16
int nksr_voxel_reduce(const int32_t* order, int64_t n, const int32_t* start, const int32_t* end, int64_t n_vox, const float* xyz,
                      const float* attr, int C, int group, float* mean_xyz_out, float* mean_attr_out, int32_t* count_out,
                      int32_t* nearest_out, void* stream);

/* ---- dual marching cubes (field.extract_dual_mesh, examples/recons_simple.py:27) ------- */
/* flags[i]=1 where voxel i and its +x,+y,+z,... 7 partners are all active */
int nksr_base_cell_flags(const int32_t* nbr, int32_t n, int32_t* flags, void* stream);
/* expand selected base voxels into U^3 lattice cell keys */
int nksr_base_cell_keys(const int32_t* ijk, const int32_t* sel, int64_t nsel, int upsample, int64_t* cell_keys, void* stream);
/* Lattice cells covered by the dual cells of the selected level-`level` voxels ((upsample << level)^3 keys each): the part of
 * the dual grid that comes from levels 1 .. adaptive_depth-1 where the finest level is absent
 * (LayerField(dec_svh, adaptive_depth), models/nksr_net.py:132; adaptive_depth 2: configs/carla/train.yaml:6). */
int nksr_level_cell_keys(const int32_t* ijk, const int32_t* sel, int64_t nsel, int level, int upsample, int64_t* cell_keys, void* stream);
/* 8 corner lattice keys per cell */
int nksr_cell_corner_keys(const int64_t* cell_keys, int64_t ncell, int64_t* corner_keys, void* stream);
/* lattice key -> position x = g*h + half_w0 */
int nksr_lattice_positions(const int64_t* vkeys, int64_t n, float h, float half_w0, float* xyz_out, void* stream);
/* sorted-key lower-bound lookup (exact match required; -1 otherwise) */
int nksr_sorted_lookup(const int64_t* sorted, int64_t n, const int64_t* q, int64_t nq, int32_t* idx_out, void* stream);
/* rank of every element of the ASCENDING list q in the ascending list `sorted`: rank_out[i] = #{ sorted < q[i] } (upper == 0) or
 * #{ sorted <= q[i] } (upper != 0) -- the merge of two sorted site lists without sorting them again (KernelField.solve: the shared
 * Morton-ordered row list of the position and the normal sites, models/nksr_net.py:105-112).  n < 2^31. */
int nksr_rank_sorted(const int64_t* sorted, int64_t n, const int64_t* q, int64_t nq, int upper, int32_t* rank_out, void* stream);
/* per cell: 8-bit sign configuration (bit c set iff f[corner c] > 0) and triangle count */
int nksr_cell_config(const int32_t* corner_idx, const float* f, int64_t ncell, int32_t* config, int32_t* ntri, void* stream);
/* flags[i]=1 where the cell's corners do not share a sign (MISE candidates) */
int nksr_cell_active_flags(const int32_t* config, int64_t ncell, int32_t* flags, void* stream);
/* ordered stream compaction: per-256-block counts, then (after an exclusive scan of the
 * counts) ordered scatter of the flagged indices -- wave ballot + popcount prefix */
int nksr_compact_block_counts(const int32_t* flags, int64_t n, int32_t* block_counts, void* stream);
int nksr_compact_scatter(const int32_t* flags, int64_t n, const int32_t* block_offsets, int32_t* sel, void* stream);
/* MISE hanging-vertex constraint: a refined vertex on a coarse edge / face gets the mean of the coarse
 * end points / face corners unless every coarse cell sharing that edge / face was refined (f_fine is updated in
 * place) -- closes T-junction cracks between refined and unrefined cells.  The coarse lattice vertices (key -> index into
 * f_coarse) and the refined coarse cells are given as nksr_hash_build tables. */
int nksr_mise_constrain(const int64_t* vkeys_fine, int64_t nv, float* f_fine, const int64_t* chash_keys, const int32_t* chash_vals,
                        int32_t chash_cap, const float* f_coarse, const int64_t* ahash_keys, const int32_t* ahash_vals,
                        int32_t ahash_cap, void* stream);
/* The same rule BEFORE the evaluation -- the replacement depends on the coarse level alone: f_fine [nv] receives the replaced values
 * and only those, flag_out [nv] = 1 exactly where nksr_mise_constrain leaves the evaluated value in place (a cell centre, every
 * adjacent coarse cell refined, a coarse vertex missing).  The field is then evaluated at the flagged vertices alone:
 * nksr_gather_rows3_f32 of their positions, nksr_scatter_f32 of their values. */
int nksr_mise_constrain_first(const int64_t* vkeys_fine, int64_t nv, float* f_fine, const int64_t* chash_keys, const int32_t* chash_vals,
                              int32_t chash_cap, const float* f_coarse, const int64_t* ahash_keys, const int32_t* ahash_vals,
                              int32_t ahash_cap, int32_t* flag_out, void* stream);
/* dst [nsel, 3] = src [sel[i], 0..2];  dst [sel[i]] = src [i] -- sel: distinct int32 row indices */
int nksr_gather_rows3_f32(const float* src, const int32_t* sel, int64_t nsel, float* dst, void* stream);
int nksr_scatter_f32(const float* src, const int32_t* sel, int64_t nsel, float* dst, void* stream);
/* children of the flagged cells: out has 8 keys per selected cell */
int nksr_cell_children(const int64_t* cell_keys, const int32_t* sel, int64_t nsel, int64_t* child_keys, void* stream);
/* triangle emission: edge keys (lower vertex index*3+axis) [ntri_total,3] */
int nksr_mc_emit(const int32_t* corner_idx, const int32_t* config, const int32_t* tri_offset, int64_t ncell,
                 int64_t* edge_keys, void* stream);
/* mesh vertices from unique edge keys (vhash: nksr_hash_build table of vkeys) */
int nksr_mc_vertices(const int64_t* edge_keys, int64_t nedge, const int64_t* vkeys, const int64_t* vhash_keys, const int32_t* vhash_vals,
                     int32_t vhash_cap, const float* vpos, const float* f, float h, float* verts_out, void* stream);
/* The same mesh without the key stream.  The edge key of nksr_mc_emit, corner index * 3 + axis, is a slot p in [0, 3 nv); the id of an
 * edge -- its rank among the sorted unique keys -- is the exclusive sum of used[] at p.
 * Sequence: used [3 nv + 1] zeroed, nksr_mc_mark_edges, eid = nksr_exclusive_sum_i32 of used (its last entry = the number of edges),
 * nksr_mc_faces, nksr_mc_edge_vertices.  3 nv < 2^31.
 * mark: used[p] = 1 and far_out[p] = the corner index of the edge's far end for every edge a triangle names (far_out [3 nv], written
 * where used; cells that share an edge store the same values: plain stores).
 * faces_out [ntri_total, 3] int32 = eid at the positions nksr_mc_emit writes its keys.
 * vertices: row eid[p] of verts_out [ne, 3], edge_vkey_out [ne] (lattice key of the lower end) and edge_axis_out [ne] for every used
 * slot p < nslot = 3 nv, by the arithmetic of nksr_mc_vertices. */
int nksr_mc_mark_edges(const int32_t* corner_idx, const int32_t* config, int64_t ncell, int32_t* used, int32_t* far_out, void* stream);
int nksr_mc_faces(const int32_t* corner_idx, const int32_t* config, const int32_t* tri_offset, int64_t ncell, const int32_t* eid,
                  int32_t* faces_out, void* stream);
int nksr_mc_edge_vertices(const int32_t* used, const int32_t* eid, const int32_t* far_in, int64_t nslot, const int64_t* vkeys,
                          const float* vpos, const float* f, float h, float* verts_out, int64_t* edge_vkey_out, int8_t* edge_axis_out,
                          void* stream);

/* ---- marching cubes on the ADAPTIVE dual graph: cells as large as their hierarchy level (field.extract_dual_mesh with
 * LayerField(dec_svh, adaptive_depth), reference models/nksr_net.py:132,214,284; specification: oracle/dual_adaptive.py) ----------
 * A primal cell is (lam, C): size 2^lam fine units, minimum corner C * 2^lam; its key = Morton(C + 2^20).  The cells of all sizes
 * form ONE table, smallest first, each size sorted by key (id = offset[l] + rank); nksr_cell_table_t names the per-size key hashes
 * (nksr_hash_build). */
#define NKSR_CELL_SIZES 12
typedef struct {
    int32_t nlev;
    int32_t lam[NKSR_CELL_SIZES];
    int32_t offset[NKSR_CELL_SIZES];
    int32_t hcap[NKSR_CELL_SIZES];
    const int64_t* hkeys[NKSR_CELL_SIZES];
    const int32_t* hvals[NKSR_CELL_SIZES];
} nksr_cell_table_t;
/* keys of k - 1 for the eight corners k of every cell of ONE size (fine coordinates): out has 8 keys per cell */
int nksr_adaptive_corner_keys(const int64_t* cell_keys, int64_t ncell, int lam, int64_t* corner_keys_out, void* stream);
/* the dual cell of every corner: cidx_out [ncorner, 8] = id of the cell that contains the fine voxel (k - 1) + o, o = (c >> 2, (c >> 1) & 1,
 * c & 1), or -1 (the smallest size is asked first) */
int nksr_adaptive_dual_cells(const int64_t* corner_keys, int64_t ncorner, const nksr_cell_table_t* table, int32_t* cidx_out, void* stream);
/* cell centres: fl(fl(C 2^lam * u) + 2^lam * (u / 2)) per axis (the lattice positions of nksr_lattice_positions in the uniform case) */
int nksr_adaptive_positions(const int64_t* cell_keys, const int32_t* cell_lam, int64_t ncell, float u, float* xyz_out, void* stream);
/* triangle emission: vertex names (A << 33) | (axis << 31) | B -- the cells the cube edge joins, A on the low side -- [ntri_total, 3] */
int nksr_mc_emit_pairs(const int32_t* corner_idx, const int32_t* config, const int32_t* tri_offset, int64_t ncell, int64_t* pair_keys,
                       void* stream);
/* mesh vertices from unique vertex names: pA + t (pB - pA), t = fA / (fA - fB), pB - pA exact from the integer coordinates */
int nksr_pair_vertices(const int64_t* pair_keys, int64_t npair, const int64_t* cell_keys, const int32_t* cell_lam, const float* cell_pos,
                       const float* f, float u, float* verts_out, void* stream);


/* ---- mesh metrics (metrics.MeshEvaluator, reference models/nksr_net.py:298-310; nksr_amd/metrics.py) ----------------------------
 * Faces are [nf, 3] vertex indices, int32 (faces_int64 = 0) or int64 (faces_int64 != 0); a face with an index outside [0, nv) counts
 * as a face of zero area.  n_points > 0 with zero faces, NULL arrays and negative sizes are argument errors. */
/* per face: unit normal (fp32, 0 for a zero-area face) and area (fp64, from the fp32 vertices); the CDF of the sampler is the inclusive
 * fp64 sum of the areas (nksr_inclusive_sum_f64) */
int nksr_mesh_face_areas(const float* v, int64_t nv, const void* faces, int faces_int64, int64_t nf, float* normal_out, double* area_out,
                         void* stream);
/* bitwise-reproducible inclusive fp64 prefix sum (rocPRIM deterministic scan; tmp / tmp_bytes as nksr_exclusive_sum_i32) */
int nksr_inclusive_sum_f64(void* tmp, size_t* tmp_bytes, const double* in, double* out, int64_t n, void* stream);
/* n area-uniform samples of the mesh.  Sample i is a pure function of (seed, i): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32)
 * and counter (i & 0xffffffff, i >> 32, 0, 0) gives the words r0..r3;
 *   u0 = ((r0 << 21) ^ (r1 >> 11)) 2^-53 picks the face: the first j with cdf[j] > u0 cdf[nf - 1] (a zero-area face is never picked);
 *   u1 = r2 2^-32, u2 = r3 2^-32, s = sqrt(u1):  x = (1 - s) a + s (1 - u2) b + s u2 c  (fp64, rounded to fp32 once);
 * normal_out[i] = face_normal[j], face_out[i] = j.  cdf [nf] from nksr_inclusive_sum_f64 over the areas (total > 0). */
int nksr_mesh_sample(const float* v, int64_t nv, const void* faces, int faces_int64, int64_t nf, const double* cdf, const float* face_normal,
                     int64_t n, uint64_t seed, float* xyz_out, float* normal_out, int64_t* face_out, void* stream);
/* Exact nearest neighbour of every query in the cloud of `pyramid` (k = 1 over the octree of nksr_sdf_from_points_pyramid; a query the
 * search cannot reach -- far outside the cloud, or outside the key range -- takes a box-pruned pass over the n_top top-level cells, whose
 * sorted keys are top_keys).  Outputs, each optional (NULL): dist_out [nq] = |q - p_nn|, dot_out [nq] = |n_q . n_nn| of the unit
 * normals (0 where either normal is zero; needs normal_sorted, in the pyramid's point order, and query_normal), partials_out
 * [ceil(nq / NKSR_NN_BLOCK), NKSR_METRIC_FIELDS] = per workgroup: sum d, sum d^2, sum dot, then the counts of d <= t for t in
 * NKSR_METRIC_THRESHOLDS, all fp64, each block summed in a fixed order. */
#define NKSR_NN_BLOCK 128
#define NKSR_METRIC_NTHRESH 5
#define NKSR_METRIC_FIELDS 8
#define NKSR_METRIC_THRESHOLDS {0.01, 0.015, 0.02, 0.002, 0.1}
int nksr_nn_metrics(const nksr_knn_pyramid_t* pyramid, const int64_t* top_keys, int32_t n_top, const float* normal_sorted, const float* query,
                    const float* query_normal, int64_t nq, int max_ring, float* dist_out, float* dot_out, double* partials_out, void* stream);
/* out [NKSR_METRIC_FIELDS] = the column sums of partials [nrows, NKSR_METRIC_FIELDS], one workgroup, fixed order (no atomics) */
int nksr_metric_reduce(const double* partials, int64_t nrows, double* out, void* stream);

/* ---- mesh queries (nksr_amd/mesh_query.py: MeshQuery, the o3d-iou of metrics.MeshEvaluator; reference metrics.py:182-190) -------
 * A linear BVH over the triangles (Karras, HPG 2012), built in four steps: nksr_bvh_morton (codes of the face centroids in the box of
 * the vertices), nksr_sort_pairs_u64_u32 (code, face index), nksr_bvh_nodes, nksr_bvh_refit.  The same input gives the same tree bit
 * for bit.  Internal node i of F - 1 is NKSR_BVH_NODE_FLOATS floats: the boxes of its two children (lo xyz, hi xyz each: [0, 6) and
 * [6, 12)), then the children as int32 bits ([12], [13]; c >= 0 an internal node, c < 0 leaf ~c), then two zeros.  Leaf k (sorted
 * position) is NKSR_BVH_LEAF_FLOATS floats: the fp32 corners a, b, c, then the original face index as int32 bits, then two zeros.
 * A face with an index outside [0, nv) gets an empty box and NaN corners: it is never crossed and never nearest.  F = 1: the root is
 * leaf 0.  Queries read `depth` (the host copy of *depth_dev, which the refit writes) and refuse a tree deeper than NKSR_BVH_STACK
 * (NKSR_ERR_CAPACITY). */
#define NKSR_BVH_NODE_FLOATS 16
#define NKSR_BVH_LEAF_FLOATS 12
#define NKSR_BVH_STACK 64
#define NKSR_BVH_MAX_FACES (1ll << 30)
/* ray directions of nksr_mesh_occupancy (rays = 1, 3, 5 or 7 use the first `rays` rows): not axis-aligned, the dominant component of
 * each exactly +-1, every component a short binary fraction, so the shear of the watertight test is exact */
#define NKSR_BVH_MAX_RAYS 7
#define NKSR_BVH_RAY_DIRS {{0.5f, 0.25f, 1.0f}, {1.0f, -0.375f, 0.625f}, {-0.625f, 1.0f, -0.25f}, {-0.25f, -0.5f, -1.0f}, \
                           {-1.0f, 0.625f, -0.375f}, {0.375f, -1.0f, 0.5f}, {-0.375f, 0.75f, 1.0f}}
typedef struct {
    int64_t n_faces;           /* F: leaves; F - 1 internal nodes; 0 <= F <= 2^30 (node indices stay int32)                     */
    int32_t depth;             /* edges from the root to the deepest leaf (host copy of *depth_dev after the refit)               */
    int32_t reserved;
    float* nodes;              /* [max(F - 1, 1), NKSR_BVH_NODE_FLOATS]                                                           */
    float* leaves;             /* [F, NKSR_BVH_LEAF_FLOATS]                                                                       */
    const float* box;          /* [6] box of the vertices (lo xyz, hi xyz; nksr_bbox): the Morton frame and the culling pad       */
    int32_t* depth_dev;        /* [1] written by nksr_bvh_refit                                                                   */
} nksr_bvh_t;
/* Morton codes (21 bits per axis, quantised in box6) of the centroids of faces [n, 3] (faces != NULL) or of the points xyz[0, n)
 * (faces == NULL); index_out[i] = i.  The query kernels take such a sorted order to walk neighbouring queries together. */
int nksr_bvh_morton(const float* xyz, int64_t nv, const void* faces, int faces_int64, int64_t n, const float* box6, uint64_t* codes_out,
                    uint32_t* index_out, void* stream);
/* internal nodes from the sorted codes (equal codes split by their sorted position): child words of bvh->nodes, and parent_work
 * [2F - 1] = 2 * parent + side (internal nodes first, then the leaves) */
int nksr_bvh_nodes(const uint64_t* codes_sorted, int32_t* parent_work, const nksr_bvh_t* bvh, void* stream);
/* leaf records of the faces in `order` (the sorted face indices) and every box, bottom up: the second child to reach a node (integer
 * atomic flag) writes the node's box into its parent; flag_work [2 (F - 1)] int32 (flags, heights; zeroed here); *depth_dev = depth */
int nksr_bvh_refit(const float* v, int64_t nv, const void* faces, int faces_int64, const uint32_t* order, const int32_t* parent_work,
                   int32_t* flag_work, const nksr_bvh_t* bvh, void* stream);
/* Occupancy by ray parity: from every query, `rays` half-lines along NKSR_BVH_RAY_DIRS; every crossing counts (watertight test of
 * Woop, Benthin and Wald 2013 with exact signs and a per-edge tie-break).  inside_out[q] = 1 when more than
 * rays / 2 of the counts are odd; counts_out [nq, rays] int32 (optional).  order: NULL or a permutation of [0, nq) (the walk order;
 * results land at the query's own index). */
int nksr_mesh_occupancy(const nksr_bvh_t* bvh, const float* query, int64_t nq, const uint32_t* order, int rays, uint8_t* inside_out,
                        int32_t* counts_out, void* stream);
/* Closest point (Ericson's point-triangle routine in fp32): dist_out [nq] (inf with no faces), face_out [nq] original face index (the
 * smaller one on a tie; -1 with no faces), point_out [nq, 3]; each optional, not all NULL. */
int nksr_mesh_closest(const nksr_bvh_t* bvh, const float* query, int64_t nq, const uint32_t* order, float* dist_out, int64_t* face_out,
                      float* point_out, void* stream);

/* ---- mesh topology (nksr_amd/mesh_topology.py: MeshTopology; csrc/meshtopo.hip) ----------------------------
 * The unique-edge table of a triangle mesh and what follows from it: edge classes, connected components, per-component statistics,
 * removal of components.  Faces as in the metrics section; here a face with an index outside [0, nv) OR with two equal indices is
 * INVALID: it has no edges, its component label is -1, it is never kept, and it is counted.  nv < 2^31, nf <= NKSR_TOPO_MAX_FACES
 * (half-edge ids 3 f + k fit uint32); beyond: NKSR_ERR_ARG.  Every result is an integer (or a min / max), so every array repeats
 * bit for bit; the one floating-point sum (component areas) goes through nksr_inclusive_sum_by_key_f64.
 * Build: nksr_topo_halfedge_keys, nksr_sort_pairs_u64_u32 (end_bit = 32 + bit_length(nv); stable, so half-edges of one edge stay in
 * ascending id order), the run table of the sorted keys with none_from = the invalid faces' key (nksr_run_counts_u64,
 * nksr_exclusive_sum_i64, (read E), nksr_run_table_u64: edge e = run e, edge_start = its start_out), nksr_topo_edge_classes. */
#define NKSR_TOPO_MAX_FACES (1ll << 30)
#define NKSR_TOPO_BOUNDARY 1        /* edge classes: one incident face                                        */
#define NKSR_TOPO_INTERIOR 2        /* two, traversing the edge in opposite directions                         */
#define NKSR_TOPO_MISORIENTED 3     /* two, traversing it in the same direction                                */
#define NKSR_TOPO_NONMANIFOLD 4     /* more than two                                                           */
#define NKSR_TOPO_TOTALS 6          /* E, boundary, non-manifold, misoriented edges, invalid faces, referenced vertices */
/* per face three pairs: key = (min(a, b) << 32) | max(a, b) of half-edge k = (corner k -> corner k + 1), id = 3 f + k; an invalid face
 * writes the key (nv << 32) | nv, which sorts last.  face_valid_out [nf], vertex_ref_out [nv] (1: named by a valid face; zeroed here). */
int nksr_topo_halfedge_keys(const void* faces, int faces_int64, int64_t nf, int64_t nv, uint64_t* keys_out, uint32_t* ids_out,
                            uint8_t* face_valid_out, uint8_t* vertex_ref_out, void* stream);
/* edge e (ascending key) = run e of the sorted keys: edge_keys [E] the runs' keys, edge_start [E + 1] the sorted position of the edge's
 * first half-edge and at [E] the number of valid half-edges.  edge_v_out [E, 2] = (min, max) of the key; edge_count_out [E] incident
 * valid faces; edge_class_out [E] NKSR_TOPO_*; face_adj_out [nf, 3]: the face across half-edge k, -1 on a boundary, a non-manifold
 * edge and an invalid face; totals_out [NKSR_TOPO_TOTALS] int64 (integer atomics) */
int nksr_topo_edge_classes(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint32_t* ids_sorted, const uint64_t* edge_keys,
                           const uint32_t* edge_start, int64_t n_edges, const uint8_t* vertex_ref, int32_t* edge_v_out, int32_t* edge_count_out,
                           uint8_t* edge_class_out, int32_t* face_adj_out, int64_t* totals_out, void* stream);
/* pairs_out [n_half, 2]: (face of sorted half-edge i, face of half-edge i + 1) when both lie on one edge, else (-1, -1): the faces
 * round an edge -- a non-manifold one too -- in a chain */
int nksr_topo_face_pairs(const uint64_t* keys_sorted, const uint32_t* ids_sorted, int64_t n_half, int64_t nv, int32_t* pairs_out, void* stream);
/* Connected components of the graph (nodes [0, n), pairs [n_pairs, 2]; a pair with a negative entry, and a node with valid[i] = 0
 * (valid may be NULL), take no part).  Union-find: hooks by atomicCAS on parent (the larger root under the smaller), path halving, one
 * flatten pass; parent[i] = the MINIMUM node index of i's component whatever order the lanes ran in (-1: no part); root_flags_out
 * [n + 1] = (parent[i] == i), then a 0.  Dense labels: root_rank = nksr_exclusive_sum_i32(root_flags) (its last entry = the number of
 * components), label_out[i] = root_rank[parent[i]] or -1: ascending label = ascending minimum node index.  n < 2^31. */
int nksr_uf_components(int32_t* parent, int64_t n, const uint8_t* valid, const int32_t* pairs, int64_t n_pairs, int32_t* root_flags_out,
                       void* stream);
int nksr_uf_labels(const int32_t* parent, int64_t n, const int32_t* root_rank, int32_t* label_out, void* stream);
/* labels of the other kind of node.  from_vertices = 0: vertex_label[v] = the smallest label among the valid faces at v (-1: none);
 * from_vertices != 0: face_label[f] = vertex_label[first corner of f] (-1 for an invalid face). */
int nksr_topo_cross_labels(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint8_t* face_valid, int from_vertices,
                           int32_t* face_label, int32_t* vertex_label, void* stream);
/* counts_out [n_comp, 4] int64 (zeroed here): faces, vertices BY THEIR LABEL, edges, boundary edges of every component.  A vertex
 * where components only touch belongs to each of them: nksr_topo_shared_corners lists the corners whose face is not of the vertex's
 * label as keys (label << 32) | vertex (keys_out NULL / capacity 0: count only; *count_out = their number, unordered), and
 * nksr_topo_count_shared adds the distinct keys of the SORTED list to the vertex column. */
int nksr_topo_component_counts(const int32_t* face_label, int64_t nf, const int32_t* vertex_label, int64_t nv, const uint32_t* ids_sorted,
                               const uint32_t* edge_start, const uint8_t* edge_class, int64_t n_edges, int64_t n_comp, int64_t* counts_out,
                               void* stream);
int nksr_topo_shared_corners(const void* faces, int faces_int64, int64_t nf, int64_t nv, const int32_t* face_label, const int32_t* vertex_label,
                             uint64_t* keys_out, int64_t capacity, int64_t* count_out, void* stream);
int nksr_topo_count_shared(const uint64_t* keys_sorted, int64_t m, int64_t n_comp, int64_t* counts, void* stream);
/* box_out [n_comp, 6] = (min xyz, max xyz) over the corners of every component's faces: order-preserving integer atomics, exact */
int nksr_topo_component_boxes(const float* v, int64_t nv, const void* faces, int faces_int64, int64_t nf, const int32_t* face_label,
                              int64_t n_comp, float* box_out, void* stream);
/* inclusive fp64 sums restarted at every change of the (sorted) key, bitwise reproducible (tmp / tmp_bytes as nksr_exclusive_sum_i32) */
int nksr_inclusive_sum_by_key_f64(void* tmp, size_t* tmp_bytes, const uint64_t* keys, const double* in, double* out, int64_t n, void* stream);
/* Compaction by a per-face keep flag.  mark: face_flags_out [nf + 1] = keep && valid (then a 0), vertex_flags_out [nv + 1] = named by
 * such a face.  After nksr_exclusive_sum_i32 of both: faces_out [kept, 3] (the input's integer type, relative order kept, indices
 * rewritten), vertex_map_out [nv] int64 = new index or -1. */
int nksr_topo_compact_mark(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint8_t* face_keep, int32_t* face_flags_out,
                           int32_t* vertex_flags_out, void* stream);
int nksr_topo_compact_faces(const void* faces, int faces_int64, int64_t nf, int64_t nv, const int32_t* face_flags, const int32_t* face_offsets,
                            const int32_t* vertex_flags, const int32_t* vertex_offsets, void* faces_out, int64_t* vertex_map_out, void* stream);

/* ---- mesh geometry (nksr_amd/mesh_geometry.py: MeshGeometry; csrc/meshgeom.hip) ----------------------------
 * The vertex-centred view of the topology's edge table and what is summed over it: vertex normals, barycentric vertex areas, angle
 * defect, cotangent mean curvature, Laplacian / Taubin smoothing.  Faces, validity and the limits as in the topology section; n_edges
 * < 2^31, so that the 2 E directed entries fit the uint32 row starts.  Positions `v` are [nv, 3] fp32 (v_float64 = 0) or fp64
 * (v_float64 != 0) and are read in that precision; everything computed and stored is fp64.  No floating-point atomic: every sum runs
 * in the order of its sorted row, so every array repeats bit for bit.
 * Build: nksr_geom_directed_keys, nksr_sort_pairs_u64_u32 (end_bit = 32 + bit_length(nv)), nksr_geom_adjacency; for the corner rows
 * nksr_geom_corner_keys, nksr_sort_pairs_u64_u32 (end_bit = bit_length(nv); stable: a row's corners ascend), nksr_geom_corner_rows. */
#define NKSR_GEOM_INTERIOR 0        /* vertex kinds: referenced, on no boundary edge                            */
#define NKSR_GEOM_ON_BOUNDARY 1     /* on at least one edge of class NKSR_TOPO_BOUNDARY                         */
#define NKSR_GEOM_UNREFERENCED 2    /* named by no valid face                                                   */
#define NKSR_GEOM_FIXED 0           /* boundary modes of the smoothing step: boundary vertices stay             */
#define NKSR_GEOM_CURVE 1           /* a boundary vertex averages its neighbours over boundary edges only        */
#define NKSR_GEOM_FREE 2            /* no special case                                                          */
#define NKSR_GEOM_WEIGHT_ANGLE 0    /* vertex normal = sum of corner angle * unit face normal                   */
#define NKSR_GEOM_WEIGHT_AREA 1     /* ... of face area * unit face normal                                      */
/* per unique edge (a, b) of edges [E, 2] two pairs: keys (a << 32) | b and (b << 32) | a, both with id = the edge; [2 E] each */
int nksr_geom_directed_keys(const int32_t* edges, int64_t n_edges, int64_t nv, uint64_t* keys_out, uint32_t* ids_out, void* stream);
/* from the SORTED pairs: start_out [nv + 1] (row of vertex v = [start[v], start[v + 1]), by lower bound; start[nv] = 2 E),
 * neighbour_out [2 E] (ascending inside a row), neighbour_edge_out [2 E] the edge of the entry, neighbour_class_out [2 E] its
 * NKSR_TOPO_* class, vertex_kind_out [nv] NKSR_GEOM_* */
int nksr_geom_adjacency(const uint64_t* keys_sorted, const uint32_t* edge_ids_sorted, int64_t n_edges, int64_t nv, const uint8_t* vertex_ref,
                        const uint8_t* edge_class, uint32_t* start_out, int32_t* neighbour_out, int32_t* neighbour_edge_out,
                        uint8_t* neighbour_class_out, uint8_t* vertex_kind_out, void* stream);
/* per corner c = 3 f + k: key = its vertex, or nv for a corner of an invalid face (sorts behind every vertex); id = c; [3 nf] each */
int nksr_geom_corner_keys(const void* faces, int faces_int64, int64_t nf, int64_t nv, const uint8_t* face_valid, uint64_t* keys_out,
                          uint32_t* ids_out, void* stream);
/* start_out [nv + 1] of the SORTED corner keys; start[nv] = the number of corners of valid faces */
int nksr_geom_corner_rows(const uint64_t* keys_sorted, int64_t n_half, int64_t nv, uint32_t* start_out, void* stream);
/* per face: angle_out / cot_out [nf, 3] of corner k (atan2(|e1 x e2|, e1 . e2) and e1 . e2 / |e1 x e2| of the two edges leaving it),
 * normal_out [nf, 3] unit (0 for a face without area), area_out [nf]; an invalid face writes zeros everywhere */
int nksr_geom_faces(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint8_t* face_valid,
                    double* angle_out, double* cot_out, double* normal_out, double* area_out, void* stream);
/* weight_out [E] = the sum, over the half-edges ids_sorted[edge_start[e] .. edge_start[e + 1]) in that order, of the cotangent of the
 * corner opposite (half-edge 3 f + k: corner (k + 2) % 3 of f): every valid face on the edge, non-manifold edges included */
int nksr_geom_edge_weights(const uint32_t* ids_sorted, const uint32_t* edge_start, int64_t n_edges, int64_t nf, const double* cot,
                           double* weight_out, void* stream);
/* one gather over the corner row of every vertex; each output optional (NULL), not all: normal_out [nv, 3] = the unit vector of
 * sum weight * face normal (weight: NKSR_GEOM_WEIGHT_*; 0 where the sum vanishes), area_out [nv] = a third of the incident faces'
 * areas, angle_sum_out [nv] = the sum of the incident corner angles */
int nksr_geom_vertex_gather(const uint32_t* corner_start, const uint32_t* corner_ids, int64_t nv, int64_t nf, const double* angle,
                            const double* face_normal, const double* face_area, int weighting, double* normal_out, double* area_out,
                            double* angle_sum_out, void* stream);
/* one gather over the adjacency row: laplacian_out [nv, 3] = (1 / 2 A_i) sum_j w_ij (x_j - x_i), mean_curvature_out [nv] =
 * |laplacian| / 2 * sgn(-laplacian . vertex_normal); NaN where vertex_kind != NKSR_GEOM_INTERIOR or A_i = 0.  Each optional, not both. */
int nksr_geom_curvature(const void* v, int v_float64, int64_t nv, const uint32_t* start, const int32_t* neighbour, const int32_t* neighbour_edge,
                        int64_t n_edges, const double* edge_weight, const double* vertex_area, const double* vertex_normal,
                        const uint8_t* vertex_kind, double* laplacian_out, double* mean_curvature_out, void* stream);
/* n_steps Laplacian steps x <- x + w (mean of the row's neighbours - x) queued on the stream without a host synchronisation, over the
 * two [nv, 3] fp64 buffers: step s reads x_a and writes x_b when s is even (w = w_even), the other way round when odd (w = w_odd);
 * the result is in x_a for an even n_steps.  A vertex stays when it is NKSR_GEOM_UNREFERENCED, flagged in `fixed` [nv] (may be NULL),
 * or NKSR_GEOM_ON_BOUNDARY under NKSR_GEOM_FIXED; under NKSR_GEOM_CURVE such a vertex averages its boundary-class entries only. */
int nksr_geom_smooth(double* x_a, double* x_b, int64_t nv, const uint32_t* start, const int32_t* neighbour, int64_t n_edges,
                     const uint8_t* neighbour_class, const uint8_t* vertex_kind, const uint8_t* fixed, int boundary, int64_t n_steps,
                     double w_even, double w_odd, void* stream);

/* ---- mesh simplification (nksr_amd/mesh_simplify.py: MeshSimplifier; csrc/meshsimp.hip) ------------------
 * Quadric vertex clustering on a uniform grid: the referenced vertices of one cell become one vertex, placed where the planes of the
 * cluster's faces say; faces that lose a corner disappear.  Faces, validity and the limits as in the topology section; K < 2^31
 * clusters.  Positions as in the geometry section; `origin` points at three HOST doubles.  Everything computed is fp64 and relative to
 * the centre of the cluster's cell.  No floating-point atomic: every sum runs in the order of its sorted run, so every array repeats bit
 * for bit.
 * Build: nksr_topo_compact_mark with every face kept (vertex flags = referenced), nksr_simp_cell_keys, nksr_sort_pairs_u64_u32 (stable,
 * over the varying key bits), the run table of the sorted keys with none_from = all ones (nksr_run_counts_u64, nksr_exclusive_sum_i64,
 * (read K), nksr_run_table_u64: cluster c = run c, cluster_start = its start_out, cluster_key = run_key_out, cluster_of[ids_sorted[i]] =
 * run_of_out[i] -- ids_sorted is a permutation, an unreferenced vertex receives the -1), nksr_simp_face_remap; for the
 * duplicates two stable nksr_sort_pairs_u64_u32 (by key_c, then key_ab gathered into that order) and nksr_simp_flag_duplicates; for the
 * corner rows of the clusters nksr_geom_corner_keys / nksr_geom_corner_rows over cluster_faces with nv = K; nksr_simp_place,
 * nksr_simp_cluster_means; nksr_topo_compact_* over (representatives, cluster_faces, keep). */
#define NKSR_SIMP_MAX_INDEX (1ll << 21)     /* cell indices per axis lie in [0, 2^21)                                  */
#define NKSR_SIMP_GROUP 16          /* lanes that share one cluster in nksr_simp_place                          */
#define NKSR_SIMP_QUADRIC 0         /* placement: the regularised quadric minimiser, clamped to the cell        */
#define NKSR_SIMP_MEAN 1            /* ... the mean of the cluster's referenced vertices                        */
/* per vertex: key = i_x << 42 | i_y << 21 | i_z with i = floor((double(x) - origin) / cell_size), an fp64 subtraction followed by an
 * fp64 division; all ones where vertex_ref [nv] is 0 and where an index falls outside [0, NKSR_SIMP_MAX_INDEX) or is not a number --
 * *misfits_out counts the latter (zeroed here).  id = the vertex; [nv] each. */
int nksr_simp_cell_keys(const void* v, int v_float64, int64_t nv, const int32_t* vertex_ref, const double* origin, double cell_size,
                        uint64_t* keys_out, uint32_t* ids_out, int64_t* misfits_out, void* stream);
/* (cluster_of [nv] = rank of the vertex's key among the distinct keys, -1: all ones; cluster_start [K + 1] = sorted position of the
 * cluster's first vertex, at [K] the number of keyed vertices; cluster_key [K])
 * per face: cluster_faces_out [nf, 3] (the input's integer type) = the clusters of its corners in corner order, (0, 0, 0) for an invalid
 * face; valid_out [nf]; survives_out [nf] = valid and three distinct clusters; with a < b < c the sorted triple of a surviving face
 * key_ab_out = a << 32 | b and key_c_out = c, both 0 elsewhere (no surviving face has that pair); ids_out [nf] = the face;
 * counts_out [2] int64 = invalid faces, collapsed faces (zeroed here; integer atomics) */
int nksr_simp_face_remap(const void* faces, int faces_int64, int64_t nf, int64_t nv, const int32_t* cluster_of, void* cluster_faces_out,
                         uint8_t* valid_out, uint8_t* survives_out, uint64_t* key_ab_out, uint64_t* key_c_out, uint32_t* ids_out,
                         int64_t* counts_out, void* stream);
/* order [nf] = the faces sorted stably by key_c and then stably by key_ab: keep_out[f] = survives[f] and not the same triple as the
 * face before it in that order (of equal triples the lowest face index stays); *count_out = the duplicates (zeroed here) */
int nksr_simp_flag_duplicates(const uint32_t* order, int64_t nf, const uint64_t* key_ab, const uint64_t* key_c, const uint8_t* survives,
                              uint8_t* keep_out, int64_t* count_out, void* stream);
/* representative_out [K, 3] fp64.  With centre = origin + (i + 0.5) cell_size of the cluster's key: mean = the mean of (x - centre) over
 * vertex_ids_sorted[cluster_start[c] .. cluster_start[c + 1]) in that order.  NKSR_SIMP_QUADRIC: over the corners
 * corner_ids[corner_start[c] .. corner_start[c + 1]) (corner 3 t + k: face t, whose unit normal n and area a are recomputed; a face
 * without area adds nothing) A = sum a n n^T, b = sum a d n with d = -n . (p0 - centre); NKSR_SIMP_GROUP lanes take every 16th corner each
 * and meet in the xor butterfly 8, 4, 2, 1.  x = (A + mu tau I)^-1 (-b + mu tau mean), tau = trace A, by a 3 x 3 Cholesky factorisation;
 * x = mean when tau = 0 and under NKSR_SIMP_MEAN (the corner arrays may then be NULL).  Output: centre + clamp(x, -cell_size / 2,
 * cell_size / 2).  0 < regularisation <= 1. */
int nksr_simp_place(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint32_t* corner_start,
                    const uint32_t* corner_ids, const uint32_t* cluster_start, const uint32_t* vertex_ids_sorted, const uint64_t* cluster_key,
                    int64_t n_clusters, const double* origin, double cell_size, double regularisation, int placement,
                    double* representative_out, void* stream);
/* mean_out [K, channels] fp64 = the mean of attr [nv, channels] (fp32, or fp64 with attr_float64 != 0) over every cluster's vertex run,
 * summed in fp64 in the order of the run (ascending vertex index); one lane per entry */
int nksr_simp_cluster_means(const void* attr, int attr_float64, int64_t nv, int64_t channels, const uint32_t* cluster_start,
                            const uint32_t* vertex_ids_sorted, int64_t n_clusters, double* mean_out, void* stream);

/* ---- mesh cross-sections (nksr_amd/mesh_slice.py: MeshSlicer; csrc/meshslice.hip) -------------------------
 * One family of parallel planes { x : n . x = offsets[j] } (n a unit vector as three HOST doubles, offsets [P] fp64 on the device,
 * finite and strictly ascending) cut into points on the unique edges of the topology section's edge table, one segment per (face,
 * crossed plane) and polylines; the definition is DESIGN.md section 3.15, restated in numpy by tests/mesh_slice_ref.py.  Faces,
 * validity and the limits as in the topology section, positions as in the geometry section; N points, S segments < 2^31.  No atomics:
 * ids are exclusive scans plus offsets, every write has one writer, every floating-point sum is nksr_inclusive_sum_by_key_f64.
 * Sequence: nksr_slice_heights, nksr_slice_counts, nksr_exclusive_sum_i64 of both count arrays (read N and S), nksr_slice_points,
 * nksr_slice_segments, nksr_chain_rank over pred, nksr_exclusive_sum_i32 of rep_flags (read L), nksr_slice_rep_list, a stable
 * nksr_sort_pairs_u64_u32 of (plane_key, position) over bit_length(P) bits: polyline l = entry l, nksr_slice_polyline_sizes,
 * nksr_exclusive_sum_i32 of both size arrays, nksr_slice_polylines, nksr_inclusive_sum_by_key_f64 of both term arrays. */
/* height_out [nv] fp64 = fma(n_z, z, fma(n_y, y, n_x x)), positions widened exactly; a height that is not a number is stored as -inf
 * (such a vertex lies below every plane).  Vertex v is ABOVE plane j iff height[v] >= offsets[j]. */
int nksr_slice_heights(const void* v, int v_float64, int64_t nv, const double* normal, double* height_out, void* stream);
/* lo = the number of offsets <= the smallest height of a valid face's corners (an edge's end points), count = the number in
 * (smallest, largest]: the item crosses the planes [lo, lo + count).  An invalid face: 0, 0.  face_lo_out [nf], face_count_out [nf + 1]
 * (a closing 0, the input of the scan), edge_lo_out [n_edges], edge_count_out [n_edges + 1]; edges [n_edges, 2] = edge_v of the edge
 * table.  The offsets are staged in LDS up to 2048 planes. */
int nksr_slice_counts(const double* height, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint8_t* face_valid,
                      const int32_t* edges, int64_t n_edges, const double* offsets, int64_t n_planes, int32_t* face_lo_out,
                      int64_t* face_count_out, int32_t* edge_lo_out, int64_t* edge_count_out, void* stream);
/* point point_start[e] + (j - edge_lo[e]) for every plane j the edge e = (a, b), a < b, crosses (point_start [n_edges + 1] = the scan
 * of edge_count): points_out [N, 3] fp64 = a + t (b - a), t = (offsets[j] - h_a) / (h_b - h_a), every operation rounded on its own;
 * point_edge_out / point_plane_out [N].  by_point = 0: one lane per edge, looping over its planes; != 0: one lane per point, which finds
 * its edge by a binary search of point_start -- the same outputs. */
int nksr_slice_points(const void* v, int v_float64, int64_t nv, const double* height, const int32_t* edges, int64_t n_edges,
                      const double* offsets, int64_t n_planes, const int32_t* edge_lo, const int64_t* point_start, int64_t n_points,
                      int by_point, double* points_out, int32_t* point_edge_out, int32_t* point_plane_out, void* stream);
/* segment seg_start[f] + (j - face_lo[f]) for every plane j face f crosses (seg_start [nf + 1] = the scan of face_count):
 * segments_out [S, 2] = (tail, head) = the points on the face's half-edge that goes above -> below and on the one that goes
 * below -> above (half-edge k runs corner k -> corner k + 1; halfedge_edge [3 nf] = its unique edge); segment_face_out,
 * segment_plane_out [S]; succ_out [S] = the segment of the same plane in face_adj[f, k] across the half-edge k that carries the head
 * when that edge's class is NKSR_TOPO_INTERIOR, else -1; pred_out [S] likewise across the half-edge that carries the tail (succ is
 * injective and pred its inverse). */
int nksr_slice_segments(const double* height, int64_t nv, const void* faces, int faces_int64, int64_t nf, const double* offsets,
                        int64_t n_planes, const int32_t* halfedge_edge, const uint8_t* edge_class, const int32_t* face_adj,
                        const int32_t* face_lo, const int64_t* seg_start, const int32_t* edge_lo, const int64_t* point_start,
                        int64_t n_segments, int32_t* segments_out, int32_t* segment_face_out, int32_t* segment_plane_out, int32_t* succ_out,
                        int32_t* pred_out, void* stream);
/* List ranking of n < 2^31 elements linked by pred [n] (the element one step nearer the start of its list; < 0, >= n or the element
 * itself: none), where no two elements share a predecessor -- the inverse of any injective successor array.  The lists are open
 * chains and cycles.  rep_out [n] = the representative: a chain's element without predecessor, a cycle's smallest element;
 * rank_out [n] = the number of steps from the representative; cyclic_out [n] = 1 on a cycle; rep_flags_out [n + 1] = (rep == the
 * element), then a 0 -- the input of nksr_exclusive_sum_i32, whose last entry is the number of lists.  Pointer doubling over two
 * ping-pong buffers of 16 bytes per element (work: 32 n bytes, 16-byte aligned): nksr_chain_rank_rounds(n) = ceil(log2 n) + 1 rounds
 * queued back to back, nothing is read on the host; chains and cycles are ranked in the same sweep (a window minimum with its distance
 * finds and cuts a cycle at its smallest element).  The outputs are a function of pred alone. */
int64_t nksr_chain_rank_rounds(int64_t n);
int nksr_chain_rank(const int32_t* pred, int64_t n, void* work, int32_t* rep_out, int32_t* rank_out, uint8_t* cyclic_out,
                    int32_t* rep_flags_out, void* stream);
/* the representatives in ascending segment id: list_out[rep_dense[s]] = s and plane_key_out[rep_dense[s]] = segment_plane[s] where
 * rep_flags[s] (rep_dense = the exclusive scan of rep_flags); [L] each */
int nksr_slice_rep_list(const int32_t* rep_flags, const int32_t* rep_dense, int64_t n_segments, const int32_t* segment_plane,
                        int64_t n_polylines, int32_t* list_out, uint64_t* plane_key_out, void* stream);
/* segment_polyline_out [S] = polyline_of_dense[rep_dense[rep[s]]]; the last segment of a polyline (no successor, or its successor is
 * the representative) writes n_segments_out[l] = m = rank + 1, n_points_out[l] = m on a cycle and m + 1 on an open chain, and
 * closed_out[l]; both size arrays are [L + 1] with a closing 0 */
int nksr_slice_polyline_sizes(const int32_t* rep, const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_segments,
                              const int32_t* rep_dense, const int32_t* polyline_of_dense, int64_t n_polylines, int32_t* segment_polyline_out,
                              int32_t* n_segments_out, int32_t* n_points_out, uint8_t* closed_out, void* stream);
/* polyline_points_out[point_offset[l] + rank] = the segment's tail, and behind the last segment of an open chain its head.  At
 * segment_offset[l] + rank: term_key_out = l, length_term_out = sqrt(dx dx + dy dy + dz dz) of head - tail, area_term_out =
 * 0.5 (n_x c_x + n_y c_y + n_z c_z) with c = (tail - p0) x (head - p0), p0 the tail of segment polyline_rep[l], on a cycle and 0 on an
 * open chain; every operation rounded on its own, sums left to right.  (The offsets are the scans of the two size arrays.) */
int nksr_slice_polylines(const int32_t* segments, const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_segments,
                         const int32_t* segment_polyline, const int32_t* polyline_rep, const int32_t* segment_offset,
                         const int32_t* point_offset, int64_t n_polylines, const double* points, int64_t n_points, const double* normal,
                         int32_t* polyline_points_out, uint64_t* term_key_out, double* length_term_out, double* area_term_out, void* stream);

/* ---- mesh clipping (nksr_amd/mesh_clip.py: MeshClipper; csrc/meshclip.hip) --------------------------------
 * A mesh split along one family of parallel planes into ONE conforming mesh: the vertices are the input's followed by the points of
 * the cross-sections section as they are (point p has id nv + p), and every valid face that crosses k planes becomes 2 k + 1
 * triangles; the definition is DESIGN.md section 3.17, restated in numpy by tests/mesh_clip_ref.py.  The slab of a vertex is the
 * number of offsets <= its height, in [0, P]; part s lies between planes s - 1 and s.  No atomics: every id is an exclusive scan plus
 * a closed form, every write has one writer.  Sequence: nksr_slice_heights, nksr_slice_counts, nksr_exclusive_sum_i64 of both count
 * arrays and of face_valid (seg_start, point_start, valid_start; read N, F2 and the pieces), nksr_slice_points, nksr_clip_faces,
 * nksr_clip_attr; to explode a labelled mesh: nksr_clip_corner_keys, a stable nksr_sort_pairs_u64_u32 of the keys, nksr_run_table_u64
 * (one new vertex per run), a stable sort of the faces by label, nksr_clip_group_faces. */
/* Face f with corners (c0, c1, c2) of slabs (s0, s1, s2) is walked c0 -> c1 -> c2 -> c0; on a half-edge a -> b the points follow in
 * travel order (planes s_a .. s_b - 1 ascending, or s_a - 1 .. s_b descending), a corner belongs to the piece of its slab, a point
 * of plane j to pieces j and j + 1.  Piece s (min s .. max s) is the walk's members of s in walk order (3 to 5 of them) and is fanned
 * from its first member: (m_0, m_i, m_i+1).  Triangle ids: face_start[f] (face_start [nf + 1] = the exclusive scan of 2 k + 1 over
 * the valid faces, 0 for an invalid one; k = face_count of nksr_slice_counts) + the triangles of the earlier pieces + the position in
 * the fan.  faces_out [F2, 3], face_source_out [F2] = f, face_part_out [F2] = s.  The id of the point of plane j on half-edge i is
 * nv + point_start[halfedge_edge[3 f + i]] + (j - min(s_a, s_b)), the min being edge_lo of that edge.  by_piece = 0: one lane per
 * face, looping over its pieces; != 0: one lane per (face, piece), which finds its face by a binary search of piece_start [nf + 1] =
 * the exclusive scan of k + 1 over the valid faces (n_pieces its last entry) -- the same outputs.  nv + n_points and F2 < 2^31. */
int nksr_clip_faces(const double* height, int64_t nv, const void* faces, int faces_int64, int64_t nf, const uint8_t* face_valid,
                    const int32_t* halfedge_edge, const int64_t* point_start, int64_t n_points, const double* offsets, int64_t n_planes,
                    const int64_t* face_start, const int64_t* piece_start, int64_t n_pieces, int64_t n_faces_out, int by_piece,
                    int32_t* faces_out, int32_t* face_source_out, int32_t* face_part_out, void* stream);
/* attr_out [N, channels] fp64 = a + t (b - a) per channel of attr [nv, channels] (fp32, or fp64 with attr_float64 != 0) at the end
 * points (a, b) = edges[point_edge[p]], t = (offsets[point_plane[p]] - h_a) / (h_b - h_a): the t of nksr_slice_points, every operation
 * rounded on its own.  One lane per (point, group of 4 channels). */
int nksr_clip_attr(const void* attr, int attr_float64, int64_t nv, int64_t channels, const double* height, const int32_t* edges,
                   int64_t n_edges, const double* offsets, int64_t n_planes, const int32_t* point_edge, const int32_t* point_plane,
                   int64_t n_points, double* attr_out, void* stream);
/* keys_out [3 nf] = (labels[f] << 32) | faces[f, k] and ids_out [3 nf] = 3 f + k for the corners of faces [nf, 3] int32 with
 * labels [nf] >= 0; 3 nf < 2^31 */
int nksr_clip_corner_keys(const int32_t* faces, const int32_t* labels, int64_t nf, uint64_t* keys_out, uint32_t* ids_out, void* stream);
/* faces_out [nf, 3]: row q = the three entries of corner_vertex [3 nf] (the new vertex of every corner) of face order[q] */
int nksr_clip_group_faces(const int32_t* order, const int32_t* corner_vertex, int64_t nf, int32_t* faces_out, void* stream);

/* ---- mesh rasterisation (nksr_amd/mesh_raster.py: MeshRasterizer; csrc/meshraster.hip) -----------------------
 * A mesh rasterised along one coordinate axis onto a regular grid: x = coordinate axis_x, y = axis_y, z = the third one, all read in
 * the caller's precision (v_float64) and widened to fp64 exactly.  Pixel (i, j) of the [nx, ny] grid (flat index i ny + j, nx ny <
 * 2^31) has the centre (origin_x + (i + 0.5) pixel_size, origin_y + (j + 0.5) pixel_size), one rounded product and one rounded sum
 * each.  The definition (coverage by the signs of three edge functions with an antisymmetric tie-break, the height and the attributes
 * from the same three values) is DESIGN.md section 3.18, restated in numpy by tests/mesh_raster_ref.py.  Faces as in the topology
 * section (int32 / int64); a face is VALID when its indices are inside [0, nv) and its nine coordinates are finite.  No atomics: every
 * id is a scan plus a position, every write has one writer.  Sequence: nksr_raster_boxes, nksr_exclusive_sum_i64 of the counts (read
 * the candidates), nksr_raster_test, nksr_raster_flag_counts, nksr_exclusive_sum_i64 (read the hits), nksr_raster_compact, a stable
 * nksr_sort_pairs_u64_u32 of (pixel, hit position), nksr_run_counts_u64 / nksr_run_table_u64, nksr_raster_pixel_start,
 * nksr_raster_reduce; then nksr_raster_sample and nksr_raster_horn on the rasters. */
#define NKSR_RASTER_BLOCK 256
/* face_valid_out [nf]; box_out [nf, 4] = (i0, i1, j0, j1), the pixels floor((min - origin) / pixel_size) - 1 .. floor((max - origin) /
 * pixel_size) + 1 per axis clamped to the grid (conservative while pixel_size >= 2^-40 of the largest coordinate or origin magnitude),
 * i1 < i0 when the face is invalid or off the grid; count_out [nf + 1] = the pixels of the box, then a 0 (the input of the scan) */
int nksr_raster_boxes(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, int axis_x, int axis_y,
                      double origin_x, double origin_y, double pixel_size, int64_t nx, int64_t ny, uint8_t* face_valid_out, int32_t* box_out,
                      int64_t* count_out, void* stream);
/* One lane per candidate c < n_candidates < 2^31: its face is the last f with cand_start[f] <= c (cand_start [nf + 1] = the scan of
 * count_out), its pixel the (c - cand_start[f])-th of the face's box, j fastest.  flag_out [n_candidates] = 1 where the face covers the
 * centre, height_out [n_candidates] = ((U z_a + V z_b) + W z_c) / det there and 0 elsewhere. */
int nksr_raster_test(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, int axis_x, int axis_y,
                     double origin_x, double origin_y, double pixel_size, int64_t nx, int64_t ny, const int32_t* box, const int64_t* cand_start,
                     int64_t n_candidates, uint8_t* flag_out, double* height_out, void* stream);
/* counts_out [B + 1], B = ceil(n_candidates / NKSR_RASTER_BLOCK): the set flags of every block of candidates, then a 0 */
int nksr_raster_flag_counts(const uint8_t* flag, int64_t n_candidates, int64_t* counts_out, void* stream);
/* The hits in candidate order (which is face order), block_start [B + 1] the scan of counts_out and n_hits its last entry:
 * hit_pixel_out [n_hits] = i ny + j, hit_face_out [n_hits], hit_height_out [n_hits] */
int nksr_raster_compact(const uint8_t* flag, const double* height, const int32_t* box, const int64_t* cand_start, int64_t nf, int64_t n_candidates,
                        int64_t nx, int64_t ny, const int64_t* block_start, int64_t n_hits, uint64_t* hit_pixel_out, int32_t* hit_face_out,
                        double* hit_height_out, void* stream);
/* pixel_start_out [n_pixels + 1] = the hits on the pixels before p, from the run table (run_keys [n_runs] = the covered pixels
 * ascending, run_start [n_runs + 1]) of the sorted pixel keys */
int nksr_raster_pixel_start(const uint64_t* run_keys, const int32_t* run_start, int64_t n_runs, int64_t n_hits, int64_t n_pixels,
                            int64_t* pixel_start_out, void* stream);
/* One lane per run.  order [n_hits] = the hit of every sorted position (ascending face id within a pixel: the sort is stable).
 * layer_face_out / layer_height_out [n_hits] = the hits in sorted order; per covered pixel count_out = the length of its run,
 * height_out = the largest (bottom != 0: the smallest) height of the run, face_out = the lowest face id that attains it.  The pixels
 * without a run are not written: the caller fills the rasters with NaN / -1 / 0 first. */
int nksr_raster_reduce(const uint64_t* run_keys, const int32_t* run_start, int64_t n_runs, const int32_t* order, const int32_t* hit_face,
                       const double* hit_height, int64_t n_hits, int bottom, int64_t n_pixels, int32_t* layer_face_out, double* layer_height_out,
                       double* height_out, int32_t* face_out, int32_t* count_out, void* stream);
/* attr_out [nx ny, channels] fp64 = ((U t_a + V t_b) + W t_c) / det per channel of attr [nv, channels] (fp32, or fp64 with
 * attr_float64 != 0) at the centre of every pixel, U, V, W recomputed for the face face_map [nx ny] names; NaN where face_map < 0.
 * One lane per (pixel, group of 4 channels). */
int nksr_raster_sample(const void* v, int v_float64, int64_t nv, const void* faces, int faces_int64, int64_t nf, int axis_x, int axis_y,
                       double origin_x, double origin_y, double pixel_size, int64_t nx, int64_t ny, const int32_t* face_map, const void* attr,
                       int attr_float64, int64_t channels, double* attr_out, void* stream);
/* Horn's differences of height [nx, ny]: gx = (((h[i+1,j-1] + 2 h[i+1,j]) + h[i+1,j+1]) - ((h[i-1,j-1] + 2 h[i-1,j]) + h[i-1,j+1])) /
 * (8 pixel_size), gy the same along j, shade = max(0, (s_z - (s_x gx + s_y gy)) / sqrt((1 + gx gx) + gy gy)) for sun = (s_x, s_y, s_z);
 * NaN on the rim and where one of the nine heights is not finite.  Every operation rounded on its own. */
int nksr_raster_horn(const double* height, int64_t nx, int64_t ny, double pixel_size, const double* sun, double* gx_out, double* gy_out,
                     double* shade_out, void* stream);

/* ---- mesh boundary loops and hole filling (nksr_amd/mesh_boundary.py: MeshBoundary; csrc/meshbound.hip) ----
 * The boundary half-edges of the topology section's edge table ordered into loops, their measures, and the faces that close them; the
 * definition is DESIGN.md section 3.16, restated in numpy by tests/mesh_boundary_ref.py.  Faces, validity and the limits as in the
 * topology section, positions as in the geometry section; halfedge_edge [3 nf] = the unique edge of half-edge 3 f + k (corner k ->
 * corner k + 1), -1 for an invalid face.  B boundary half-edges, L loops.  No floating-point atomic: ids are exclusive scans plus
 * offsets, every write has one writer, every floating-point sum is nksr_inclusive_sum_by_key_f64; the boxes are integer min / max.
 * Sequence: nksr_bnd_flags, nksr_exclusive_sum_i32 (boundary_of; its last entry is B), nksr_bnd_list, nksr_bnd_successor,
 * nksr_chain_rank over pred, nksr_exclusive_sum_i32 of rep_flags (read L), nksr_bnd_loop_sizes, nksr_exclusive_sum_i32 of both size
 * arrays, nksr_bnd_terms, nksr_inclusive_sum_by_key_f64 of the seven term rows, nksr_bnd_boxes; to fill: nksr_bnd_fill and
 * nksr_bnd_fill_vertices. */
/* flags_out [3 nf + 1] = 1 where the half-edge's unique edge has class NKSR_TOPO_BOUNDARY, then a 0 (the input of the scan) */
int nksr_bnd_flags(const int32_t* halfedge_edge, const uint8_t* edge_class, int64_t nf, int64_t n_edges, int32_t* flags_out, void* stream);
/* boundary id b = boundary_of[h] (the exclusive scan of flags) of every flagged half-edge h = 3 f + k: halfedge_out [B] = h,
 * tail_out / head_out [B] = corners k and k + 1 of f, face_out [B] = f */
int nksr_bnd_list(const void* faces, int faces_int64, int64_t nf, const int32_t* flags, const int32_t* boundary_of, int64_t n_boundary,
                  int32_t* halfedge_out, int32_t* tail_out, int32_t* head_out, int32_t* face_out, void* stream);
/* succ_out [B]: rotation about the head b of (a -> b) in f: the next half-edge (b -> c) of the face; BOUNDARY: its boundary id; INTERIOR:
 * cross to face_adj, find the corner that holds (c -> b), continue with the half-edge after it; any other class: -1.  pred_out [B]: the
 * mirrored walk about the tail.  succ is injective and pred its inverse; a walk takes at most valence steps and needs no guard. */
int nksr_bnd_successor(const void* faces, int faces_int64, int64_t nf, const int32_t* halfedge_edge, const uint8_t* edge_class,
                       const int32_t* face_adj, const int32_t* boundary_of, const int32_t* halfedge, int64_t n_boundary, int32_t* succ_out,
                       int32_t* pred_out, void* stream);
/* rep / rank / cyclic of nksr_chain_rank over pred, rep_dense the scan of its rep_flags: boundary_loop_out [B] = rep_dense[rep[b]] (loop
 * ids ascend by representative), loop_rep_out [L]; the last half-edge of a loop writes loop_edges_out[l] = m = rank + 1,
 * loop_points_out[l] = m on a cycle and m + 1 on an open chain, and closed_out[l]; both size arrays are [L + 1] with a closing 0 */
int nksr_bnd_loop_sizes(const int32_t* rep, const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_boundary,
                        const int32_t* rep_dense, int64_t n_loops, int32_t* boundary_loop_out, int32_t* loop_rep_out, int32_t* loop_edges_out,
                        int32_t* loop_points_out, uint8_t* closed_out, void* stream);
/* loop_halfedges_out[edge_offset[l] + rank] = the half-edge, loop_vertices_out[point_offset[l] + rank] = its tail, and behind the last
 * half-edge of an open chain its head.  terms_out [7, B] at column edge_offset[l] + rank, with p the tail, q the head, p0 the tail of
 * loop_rep[l], a = p - p0, c = q - p0: row 0 w = sqrt(dx dx + dy dy + dz dz) of q - p; rows 1..3 0.5 (a x c) on a cycle, 0 on an open
 * chain; rows 4..6 w (0.5 (a + c)); term_key_out = l there.  Every operation rounded on its own. */
int nksr_bnd_terms(const void* v, int v_float64, int64_t nv, const int32_t* halfedge, const int32_t* tail, const int32_t* head,
                   const int32_t* rank, const uint8_t* cyclic, const int32_t* succ, int64_t n_boundary, const int32_t* boundary_loop,
                   const int32_t* loop_rep, const int32_t* edge_offset, const int32_t* point_offset, int64_t n_loops,
                   int32_t* loop_halfedges_out, int32_t* loop_vertices_out, uint64_t* term_key_out, double* terms_out, void* stream);
/* box_out [L, 6] fp64 = (min xyz, max xyz) over the tails and heads of every loop, by 64-bit order-preserving integer atomicMin /
 * atomicMax in work [L, 6] (any contents) */
int nksr_bnd_boxes(const void* v, int v_float64, int64_t nv, const int32_t* tail, const int32_t* head, const int32_t* boundary_loop,
                   int64_t n_boundary, int64_t n_loops, uint64_t* work, double* box_out, void* stream);
/* The new faces of the loops with keep[l] != 0, into faces_out [n_new_faces, 3] (int32, or int64 with faces_int64 != 0), appended loop
 * by loop from face_offset[l], in rank order; face_loop_out [n_new_faces] = l.  method 0 ('centroid'): the half-edge (a -> b) of rank r
 * gives face face_offset[l] + r = (b, a, nv + kept_rank[l]).  method 1 ('fan'): for 1 <= r <= m - 2 face face_offset[l] + r - 1 =
 * (b, a, p0), p0 the tail of loop_rep[l].  Both wind against the boundary half-edges. */
int nksr_bnd_fill(const int32_t* tail, const int32_t* head, const int32_t* rank, const int32_t* boundary_loop, int64_t n_boundary,
                  const int32_t* loop_rep, const int32_t* loop_edges, const uint8_t* keep, const int32_t* kept_rank, const int32_t* face_offset,
                  int64_t n_loops, int method, int64_t nv, int64_t n_new_faces, void* faces_out, int faces_int64, int32_t* face_loop_out,
                  void* stream);
/* v_out [n_kept, 3] (fp32, or fp64 with v_float64 != 0): row kept_rank[l] = loop_centroid[l] cast once; color_mean_out [n_kept,
 * channels] fp64 = the mean of colors [nv, channels] (fp32, or fp64 with colors_float64 != 0) over the loop's vertices, summed in fp64
 * in rank order (channels = 0: colors and color_mean_out NULL).  One lane per (loop, output column). */
int nksr_bnd_fill_vertices(const double* loop_centroid, const int32_t* point_offset, const int32_t* loop_vertices, const int32_t* loop_edges,
                           const uint8_t* keep, const int32_t* kept_rank, int64_t n_loops, int64_t n_kept, const void* colors,
                           int colors_float64, int64_t channels, int64_t nv, void* v_out, int v_float64, double* color_mean_out,
                           void* stream);

/* ---- normal orientation without sensors (csrc/orient.hip; nksr_amd/orient.py orient_graph) -------------
 * Hoppe et al. 1992: the minimum spanning forest of the k-nearest-neighbour graph under the weight 1 - |n_i . n_j|, sign flips
 * propagated along it.  DEFINITION (restated in tests/orient_ref.py; every output is a function of the input alone):
 *   input    xyz [n, 3], normal [n, 3] fp32 (finite, any sign, |component| < 2^60), idx [n, k] int32, 1 <= k <= 32, n < 2^31,
 *            n k < 2^32.  An entry of idx that is < 0, >= n or equal to its row index is ignored; duplicates are allowed.  The directed
 *            slot s = i k + c stands for the undirected edge {i, idx[i, c]}.
 *   dot      dot(a, b) = fl32(fl32(fl32(a0 b0) + fl32(a1 b1)) + fl32(a2 b2)): round-to-nearest products and sums, never fused
 *            (symmetric in a, b; np.float32 arithmetic gives the same bits).
 *   weight   w = max(fl32(1 - |dot(n_i, n_j)|), 0);  flip bit of the edge = dot(n_i, n_j) < 0.
 *   key      (bits(w) << 32) | s, 64 bits: w >= 0, so its bit pattern orders as an unsigned integer, and no two slots share a key: the
 *            minimum spanning forest of the multigraph of all slots -- a slot counts for the components of BOTH its end points, so the
 *            graph is the symmetrised one although idx is not symmetric -- is unique.
 *   relative sign of a point = XOR of the edge flip bits along the forest path to a fixed point of its component.
 *   global sign of a component, mode 0 ('+z'): its point of largest z (-0 counts as +0; the lowest index on a tie) ends with n_z >= 0;
 *            mode 1 (viewpoint v): with t = fl32(v - x) per axis, its point of smallest dot(t, t) (the lowest index on a tie) ends with
 *            dot(n, t) >= 0.
 *   outputs  flipped [n] uint8, normal_out = flipped ? -normal : normal, and the component of every point.
 * One Boruvka round (the host loops until one component is left or a round hooks nothing; Python: orient._forest):
 *   propose  every slot of a point that is not `done` and whose end points lie in different components takes the 64-bit minimum of
 *            its key into best[] of both components' representatives (rep [n]; best [n] starts as all ones).  The lanes of a wavefront
 *            that share a representative reduce their keys first.  A point whose neighbours all share its component is marked done
 *            for good.  order [n] (may be NULL) = the point every thread takes (a Morton order keeps a wavefront inside one component).
 *            counters[1] += points still active.
 *   hook     every representative r with a finite best[r] links to the representative on the other side of that slot, with the parity
 *            par[u] ^ par[v] ^ flip(u, v); two representatives that chose the same slot: the lower one stays a root.  link / lpar [n]
 *            are written for representatives only (a root links to itself, parity 0).  counters[0] += links made.
 *   jump     one pointer-doubling step over the representatives: link_out[r] = link_in[link_in[r]], parities XORed; ping-pong buffers,
 *            ceil(log2(links made)) steps flatten every chain.
 *   relabel  rep[i] = link[rep[i]], par[i] ^= lpar[rep[i]], best[i] = all ones.
 * After the loop: seeds (seed_key [n] zeroed, min_index [n] filled with 0x7FFFFFFF beforehand): per representative the 64-bit maximum of
 * (ordered key << 32) | ~index over its points and the minimum point index; apply: the outputs, parent_out[i] = the minimum index of
 * i's component and root_flags_out [n + 1] = (parent_out[i] == i), then a 0 -- the inputs of nksr_exclusive_sum_i32 / nksr_uf_labels,
 * so dense ids ascend with the components' minimum point index. */
#define NKSR_ORIENT_MAX_K 32
#define NKSR_ORIENT_SEED_Z 0
#define NKSR_ORIENT_SEED_VIEWPOINT 1
int nksr_orient_init(int64_t n, int32_t* rep, uint8_t* par, uint8_t* done, uint64_t* best, void* stream);
int nksr_orient_propose(const float* normal, const int32_t* idx, int64_t n, int k, const int32_t* order, const int32_t* rep, uint8_t* done,
                        uint64_t* best, int32_t* counters, void* stream);
int nksr_orient_hook(const float* normal, const int32_t* idx, int64_t n, int k, const int32_t* rep, const uint8_t* par, const uint64_t* best,
                     int32_t* link_out, uint8_t* lpar_out, int32_t* counters, void* stream);
int nksr_orient_jump(const int32_t* rep, int64_t n, const int32_t* link_in, const uint8_t* lpar_in, int32_t* link_out, uint8_t* lpar_out,
                     void* stream);
int nksr_orient_relabel(int64_t n, int32_t* rep, uint8_t* par, const int32_t* link, const uint8_t* lpar, uint64_t* best, void* stream);
int nksr_orient_seeds(const float* xyz, int64_t n, const int32_t* rep, int mode, float vx, float vy, float vz, uint64_t* seed_key,
                      int32_t* min_index, void* stream);
int nksr_orient_apply(const float* xyz, const float* normal, int64_t n, const int32_t* rep, const uint8_t* par, const uint64_t* seed_key,
                      const int32_t* min_index, int mode, float vx, float vy, float vz, uint8_t* flipped_out, float* normal_out,
                      int32_t* parent_out, int32_t* root_flags_out, void* stream);

/* ---- moving-least-squares projection (csrc/mls.hip; nksr_amd/mls.py: cloud.mls_project, cloud.smooth_mls) ----------------------------
 * Every query q is projected onto a polynomial fitted to its neighbours with Gaussian weights; csrc/mls.hip states the definition in
 * full.  The grid as nksr_radius_count takes it (cell >= radius); neighbours: knn_d2(p - q) <= fl32(radius)^2, the predicate and the
 * count of nksr_radius_count; weights exp(-|p - q|^2 / sigma^2) in fp64.  normal_sorted [n_ref, 3] (fp32, the grid's order) or NULL: signs
 * the fitted normal.  query [nq, 3] or NULL: the first nq points of the sorted cloud.  order 1: the weighted least-squares plane; 2: a
 * quadric over that plane.  min_neighbors >= 3 (order 1) / 6 (order 2).  Outputs, per query: position_out [nq, 3], normal_out [nq, 3],
 * mean_curvature_out / gaussian_curvature_out / variation_out [nq] (fp64; NaN where they are not defined), count_out [nq] (int32: the
 * neighbours), order_used_out [nq] (int8): 0 = not enough neighbours or collinear ones, the point is returned as it is; 1 = the plane;
 * 2 = the quadric.  fp64 sums in a fixed order, no atomics. */
int nksr_mls_project(const float* xyz_sorted, int64_t n_ref, const int32_t* start, const int32_t* end, const int64_t* hkeys,
                     const int32_t* hvals, int32_t hcap, float cell, float inv_cell, const float* normal_sorted, const float* query,
                     int64_t nq, float radius, double sigma, int order, int min_neighbors, double* position_out, double* normal_out,
                     double* mean_curvature_out, double* gaussian_curvature_out, double* variation_out, int32_t* count_out,
                     int8_t* order_used_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
