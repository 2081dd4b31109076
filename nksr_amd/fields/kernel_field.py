"""Neural kernel field -- host-side mirror of ``nksr.fields.KernelField``.

Reference interface (call sites): ``KernelField(svh=, interpolator=, features=,
approx_kernel_grad=)`` models/nksr_net.py:91-96; ``solver_config['verbose']`` :97-98;
``solve_non_fused(pos_xyz=, normal_xyz=, normal_value=, pos_weight=, normal_weight=,
reg_weight=)`` :105-112; fused ``solve`` selected by ``fused_mode`` examples/recons_waymo.py:33;
``evaluate_f`` / ``evaluate_f_bar`` models/loss.py:99,189-198.

Math: unknowns alpha (one per voxel per level, levels
concatenated fine -> coarse), f(x) = sum_d sum_{j in N27(x)} alpha_j <phi_d(x), psi_j> B(.),
normal equations (w_p G^T G + w_n Q^T Q + reg I) alpha = w_n Q^T n solved by Jacobi-PCG.
All numeric work runs in HIP kernels (csrc/kfield.hip, gram.hip, assemble.hip, packed_rows.hip, spmv.hip, cheb.hip, pcg.hip).

This module holds the field: its API, the solve policies and the evaluation.  The set-up of a solve lives beside it:
assembly.py (CSR assembly), operator_setup.py + row_layout.py (matrix-free operator), coarse_precond.py (coarse-level
preconditioner), autograd.py (differentiable solve / evaluation).  KernelField keeps a method for each of them.

Environment switches read by these modules (diagnostics, tests and tuning; none is needed in production):
  NKSR_TIMING_DETAIL=1     synchronised sub-stage times of the set-up in DETAIL_TIMES (_timing.py; bench.py reports them)
  NKSR_ROW_FORMAT          'dense' | 'factors' | 'auto': row format of the matrix-free operator (_row_format; solver_config wins)
  NKSR_ROW_ORDER=sort      row layout by a radix sort of the concatenated keys instead of rank passes (operator_setup.py; a test pins one against the other)
  NKSR_ROWS_KERNEL=site    a row-kernel launch per site set instead of the merged launch (operator_setup.py; bit-identical rows)
  NKSR_PC_LEVEL / NKSR_PC_STEPS / NKSR_PC_RATIO    first level, Chebyshev steps and interval ratio of the coarse-level block (coarse_precond.py; solver_config wins)
  NKSR_PC_PACKED=0         keep the coarse-level block as a plain CSR (coarse_precond.py)
  NKSR_PC_DROP             drop tolerance of the packed coarse-level block (coarse_precond.py; default PC_DROP_TOL)
  NKSR_THETA_VJP=torch     theta vector-Jacobian products through the torch statement of the kernel rows (autograd.py; the tests' reference, never a fallback)
"""
import collections
import ctypes as C
import os
import time

import torch

from .. import _lib, ops
from .._lib import HierT, SegmentsT, call, ptr, stream
from . import assembly, autograd, coarse_precond, operator_setup
from ._timing import DETAIL_TIMES, _tick        # noqa: F401  (DETAIL_TIMES: the dict _tick writes, read here by bench.py)
from .autograd import _EvaluateFunction, _SolveFunction
from .base_field import BaseField, EvaluationResult


def pack_interpolator(interp):
    """Flat fp32 weights W1[H,K] b1[H] W2[H,H] b2[H] W3[K,H] b3[K] of one level."""
    return interp.packed()


SMALL_FIELD_UNKNOWNS = 1 << 16      # single fields up to this size take the coarse-level block at once, from level 1 (solve_fused)
SMALL_FIELD_CHECK_EVERY = 6
SMALL_FIELD_PC = {'first_level': 1, 'steps': 8, 'ratio': 40.0}


class SiteSet(collections.namedtuple('SiteSet', 'xs keys perm target sw rows grad')):
    """One constraint site set prepared for a solve (KernelField._site_sets): Morton-sorted coordinates, their level-0 keys, the
    permutation that sorted them (None: they came sorted), the caller's targets (unsorted, unscaled), sqrt(weight) (a float, or
    one per site), the rows a site owns and whether they are gradient rows."""
    __slots__ = ()

    @property
    def scale(self):
        return 1.0 if torch.is_tensor(self.sw) else self.sw

    @property
    def site_scale(self):
        return self.sw if torch.is_tensor(self.sw) else None


class Segments:
    """Independent diagonal blocks of ONE hierarchy (nksr_segments_t): the chunks of a batched chunk solve.  Segment i owns
    the Morton key range [key_lo[i], key_hi[i]) of the finest level (an aligned cube of the lattice: its ancestors' ranges are the
    shifted ones), hence one contiguous run of voxels per level and one contiguous run of the Morton-sorted sites.  Everything is
    derived on the device (searchsorted), no host sync."""

    def __init__(self, svh, key_lo, key_hi, ids=None):
        dev = svh.device
        self.key_lo, self.key_hi = key_lo.to(dev, torch.int64).contiguous(), key_hi.to(dev, torch.int64).contiguous()
        self.nseg, self.nranges = int(self.key_lo.numel()), svh.depth
        self.ids = list(ids) if ids is not None else list(range(self.nseg))
        off = svh.offsets
        lo, hi, segs = [], [], []
        for d in range(svh.depth):
            k = svh.level(d).keys
            a = torch.searchsorted(k, self.key_lo >> (3 * d))
            b = torch.searchsorted(k, self.key_hi >> (3 * d))
            lo.append(a + off[d])
            hi.append(b + off[d])
            segs.append(torch.bucketize(k, self.key_lo >> (3 * d), right=True) - 1)
        self.lo = torch.stack(lo, 1).to(torch.int32).contiguous()          # [nseg, L]
        self.hi = torch.stack(hi, 1).to(torch.int32).contiguous()
        self.unknown_seg = torch.cat(segs).to(torch.int32).contiguous()     # [M]
        self.info = torch.zeros((self.nseg, 2), dtype=torch.float64, device=dev)
        self.c = SegmentsT()
        self.c.nseg, self.c.nranges = self.nseg, self.nranges
        self.c.lo, self.c.hi, self.c.info = ptr(self.lo), ptr(self.hi), ptr(self.info)

    def of_keys(self, keys0):
        """segment of level-0 Morton keys"""
        return torch.bucketize(keys0, self.key_lo, right=True) - 1


class KernelField(BaseField):
    def __init__(self, svh, interpolator, features, approx_kernel_grad=False):
        super().__init__(svh)
        self.approx_kernel_grad = bool(approx_kernel_grad)
        self.solver_config = {'verbose': False, 'max_iter': 2000, 'tol': 1e-5, 'check_every': 16, 'sync_timing': False}
        self.solve_info = {}
        self.kdim = int(interpolator[0].kernel_dim)
        self.hidden = int(interpolator[0].hidden_dim)
        dev = svh.device
        self._mlp = [pack_interpolator(interpolator[d]).detach().to(dev, torch.float32).contiguous() for d in range(svh.depth)]
        self._interps_in, self._feat_in = list(interpolator), list(features)      # the caller's tensors / modules (autograd, training path)
        self._feat, self._psi = [], []
        for d in range(svh.depth):
            n = svh.num_voxels(d)
            f = features[d] if features[d] is not None else torch.zeros((0, self.kdim), device=dev)
            f = f.detach().to(dev, torch.float32).contiguous()
            if f.shape != (n, self.kdim):
                raise RuntimeError('basis_features[%d] has shape %s, expected (%d, %d)' % (d, tuple(f.shape), n, self.kdim))
            psi = torch.empty_like(f)
            call('nksr_voxel_psi', ptr(f), n, self.kdim, self.hidden, ptr(self._mlp[d]), ptr(psi), stream())
            self._feat.append(f)
            self._psi.append(psi)
        self._apsi_key = None
        self.alpha = torch.zeros(svh.num_unknowns, dtype=torch.float32, device=dev)
        self._hier = self._make_hier()
        self.matrix = None  # (rowptr, cols, vals, diag) of the last non-fused solve

    # alpha is written by HIP kernels through raw pointers (no torch version bump) and the caching allocator recycles
    # addresses, so the evaluation cache (_alpha_hier) is keyed on ASSIGNMENT: every ``fld.alpha = ...`` drops it
    @property
    def alpha(self):
        return self._alpha

    @alpha.setter
    def alpha(self, value):
        self._alpha = value
        self._apsi_key = None
        self._apsi = self._apsi_hier = None

    def invalidate_alpha_cache(self):
        """Call after writing into ``alpha``'s storage in place (kernels, ``alpha[...] = ``)."""
        self._apsi_key = None
        self._apsi = self._apsi_hier = None

    # ---- C struct describing the hierarchy + features ------------------------------------------
    def _make_hier(self):
        h = HierT()
        svh = self.svh
        h.depth, h.kdim, h.hidden, h.inv_w0 = svh.depth, self.kdim, self.hidden, svh.inv_w0
        off = svh.offsets
        for d in range(svh.depth):
            g = svh.level(d)
            lv = h.lv[d]
            lv.n, lv.offset = g.num_voxels, off[d]
            lv.keys, lv.ijk, lv.nbr = ptr(g.keys), ptr(g.ijk), ptr(g.nbr)
            lv.hkeys, lv.hvals, lv.hcap = ptr(g.hash.hkeys), ptr(g.hash.hvals), g.hash.cap
            lv.feat, lv.psi, lv.mlp = ptr(self._feat[d]), ptr(self._psi[d]), ptr(self._mlp[d])
        return h

    # ---- kernel rows ---------------------------------------------------------------------------------
    def kernel_rows(self, xyz, grad, scale=1.0, values=True, hier=None):
        """Dense-slot rows: val [n, L, 27] (``None`` with values=False) and (grad) dval [n, 3, L, 27]
        (model units), times ``scale``.  ``hier``: a masked copy of the hierarchy (_coarse_hier): rows of masked levels are 0."""
        n, L = xyz.shape[0], self.svh.depth
        val = torch.empty((n, L, 27), dtype=torch.float32, device=self.device) if values else None
        dval = torch.empty((n, 3, L, 27), dtype=torch.float32, device=self.device) if grad else None
        call('nksr_kernel_rows', C.byref(hier if hier is not None else self._hier), ptr(xyz), n, int(self.approx_kernel_grad), float(scale), None, 0, None, None,
             ptr(val), ptr(dval), stream())
        return val, dval

    def _coarse_hier(self, c0):
        """The hierarchy restricted to its levels >= c0: the finer levels are EMPTY (no voxels, no hash: every site misses them),
        the coarse ones keep their level index -- and with it their geometry -- and are re-based to unknown 0."""
        h = HierT.from_buffer_copy(self._hier)
        off = self.svh.offsets
        for d in range(self.svh.depth):
            if d < c0:
                h.lv[d].n, h.lv[d].offset, h.lv[d].hcap = 0, 0, 0
            else:
                h.lv[d].offset = off[d] - off[c0]
        return h

    def kernel_rows_level_major(self, xyz, grad, scale, out, level_stride, row_index=None, row_cells=None, site_scale=None):
        """Rows of the sites ``xyz`` written LEVEL-MAJOR into ``out`` ([L, level_stride, 27]): position rows (grad=False, one per
        site) or gradient rows (three per site), site i at row ``row_index[i]`` (default i * rows-per-site); ``row_cells``
        [L, level_stride] receives the level-d cell (global unknown index) of every row written."""
        call('nksr_kernel_rows', C.byref(self._hier), ptr(xyz), xyz.shape[0], int(self.approx_kernel_grad), float(scale), ptr(site_scale), int(level_stride),
             ptr(row_index), ptr(row_cells), None if grad else ptr(out), ptr(out) if grad else None, stream())

    def kernel_factors_level_major(self, xyz, grad, scale, vec, pos, level_stride, row_index=None, row_cells=None, site_scale=None):
        """The rank-4 factor records of the sites' rows (csrc/kfield.hip: k_kernel_factors; kernel_dim 4): ``vec`` [L, level_stride, 4],
        ``pos`` [level_stride, 4]; a position site owns one row, a normal site (grad=True) four (header + one per axis)."""
        call('nksr_kernel_factors', C.byref(self._hier), ptr(xyz), xyz.shape[0], int(bool(grad)), int(self.approx_kernel_grad), float(scale),
             ptr(site_scale), int(level_stride), ptr(row_index), ptr(row_cells), ptr(vec), ptr(pos), stream())

    def _row_format(self):
        """'dense' (the default: 108 bytes per row and level, the sweep streams them -- HBM-bound) or 'factors' (kernel_dim 4 only,
        opt-in by solver_config['row_format'] / NKSR_ROW_FORMAT: 16-byte records per row and level, the sweep rebuilds the 27
        slots in registers -- a fifth of the memory (8 GB instead of 38 GB on the 64-chunk scene), but bound by vector-ALU issue:
        22 ms per application there against 11 ms)."""
        want = self.solver_config.get('row_format') or os.environ.get('NKSR_ROW_FORMAT') or 'auto'
        if want not in ('auto', 'factors', 'dense'):
            raise RuntimeError("row_format must be 'auto', 'factors' or 'dense'")
        if want == 'factors' and self.kdim != 4:
            raise RuntimeError('the factor form of the kernel rows needs kernel_dim 4')
        return 'factors' if (want == 'factors' and self.kdim == 4) else 'dense'

    def _sorted_sites(self, xyz):
        """Permutation that Morton-sorts sites by their level-0 cell + the sorted keys."""
        n = xyz.shape[0]
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        call('nksr_point_keys', ptr(xyz), n, self.svh.inv_w0, ptr(keys), stream())
        idx = torch.arange(n, dtype=torch.int32, device=self.device)
        ks, perm = ops.sort_pairs(keys, idx, level=0)
        return ks, perm.long()

    def _site_ranges(self, site_keys):
        starts, ends = [], []
        for d in range(self.svh.depth):
            g = self.svh.level(d)
            s = torch.empty(g.num_voxels, dtype=torch.int32, device=self.device)
            e = torch.empty(g.num_voxels, dtype=torch.int32, device=self.device)
            call('nksr_site_ranges', ptr(site_keys), site_keys.numel(), ptr(g.keys), g.num_voxels, d, ptr(s), ptr(e), stream())
            starts.append(s)
            ends.append(e)
        return starts, ends

    def _site_sets(self, pos, normal, rows_per_normal=3, per_site_weights=False):
        """The site sets of a solve, prepared once for assemble() and fused_operator(): ``pos`` / ``normal`` =
        (xyz, target, weight, sorted keys or None).  Empty sets are left out.  ``per_site_weights``: a tensor weight holds every
        site's own sqrt(weight) (batched chunks: the weight of the site's chunk)."""
        sets = []
        for (xyz, target, weight, pre), rows in ((pos, 1), (normal, rows_per_normal)):
            if xyz is None or xyz.shape[0] == 0:
                continue
            per_site = per_site_weights and torch.is_tensor(weight)
            if not per_site and not float(weight) >= 0.0:
                raise RuntimeError('solver weights must be >= 0')
            xyz = xyz.to(self.device, torch.float32).contiguous()
            if pre is not None:
                ks, perm, xs = pre, None, xyz
            else:
                ks, perm = self._sorted_sites(xyz)
                xs = xyz[perm].contiguous()
            if per_site:
                sw = weight.to(self.device, torch.float32)
                sw = (sw[perm] if perm is not None else sw).contiguous()
            else:
                sw = float(weight) ** 0.5
            sets.append(SiteSet(xs, ks, perm, target, sw, rows, rows > 1))
        return sets

    # ---- assembly -----------------------------------------------------------------------------------
    def assemble(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight=1.0,
                 pos_sorted_keys=None, normal_sorted_keys=None, coarse_from=None, fused_op=None):
        """Materialise the CSR normal equations: (rowptr, cols, vals, diag, b) -- assembly.assemble."""
        return assembly.assemble(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight,
                                 pos_sorted_keys, normal_sorted_keys, coarse_from, fused_op)

    # ---- solve ------------------------------------------------------------------------------------------
    def solve_non_fused(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight=1.0,
                        pos_sorted_keys=None, normal_sorted_keys=None):
        """Assemble the sparse system explicitly and solve it with Jacobi-PCG."""
        from .. import solver
        t0 = time.perf_counter()
        rowptr, cols, vals, diag, b = self.assemble(pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight,
                                                    pos_sorted_keys, normal_sorted_keys)
        # the same preconditioner policy as the matrix-free solve: hierarchies of 5+ levels (Jacobi needs ~47 iterations per
        # tree_depth-5 chunk, the coarse-level block ~13) or an explicit solver_config['coarse_precond']
        cfg = self.solver_config
        pc = None
        if cfg.get('coarse_precond') is not False and (isinstance(cfg.get('coarse_precond'), dict) or self.svh.depth >= 5):
            pc = self._coarse_precond(None, reg_weight, sites=dict(pos_xyz=pos_xyz, normal_xyz=normal_xyz, normal_value=normal_value,
                                                                   pos_weight=pos_weight, normal_weight=normal_weight,
                                                                   pos_sorted_keys=pos_sorted_keys, normal_sorted_keys=normal_sorted_keys))
        if cfg.get('verbose') or cfg.get('sync_timing'):
            torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        x, iters, rel = solver.pcg_solve(rowptr, cols, vals, diag, b, tol=cfg['tol'], max_iter=cfg['max_iter'], check_every=cfg['check_every'],
                                         precond=pc['pc'] if pc else None)
        t2 = time.perf_counter()
        self.alpha = x
        self.matrix = (rowptr, cols, vals, diag)
        self._fused_op = None
        self._pc = pc if self._wants_grad(normal_value) else None      # the adjoint solve of the backward pass takes the same preconditioner (_solve_system)
        self.rhs, self.diag = b, diag
        self.solve_info = {'iters': iters, 'rel_residual': rel, 'M': int(b.numel()), 'nnz': int(self.nnz),
                           'coarse_precond': ({k: pc[k] for k in ('first_level', 'unknowns', 'nnz', 'steps', 'lambda', 'gershgorin')} if pc else None),
                           'jacobi_fallbacks': solver.last_fallbacks, 't_assemble': t1 - t0, 't_pcg': t2 - t1}
        self._attach_autograd(pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight)
        if self.solver_config.get('verbose'):
            print('[KernelField] M=%d nnz=%d iters=%d rel=%.3e assemble=%.3fs pcg=%.3fs' % (
                b.numel(), self.nnz, iters, rel, t1 - t0, t2 - t1))
        return self

    # ---- matrix-free ("fused") solve ---------------------------------------------------------------------
    def fused_operator(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, pos_sorted_keys=None, normal_sorted_keys=None,
                       pos_value=None, segments=None):
        """Everything the matrix-free operator needs (nksr_fused_op_t), as a dict -- operator_setup.fused_operator."""
        return operator_setup.fused_operator(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, pos_sorted_keys,
                                             normal_sorted_keys, pos_value, segments)

    def dense_rows(self, op):
        """[L, rows_total, 27] view of the dense-slot rows of a matrix-free operator (test / export helper)."""
        L, R = self.svh.depth, op['rows_total']
        return op['rows_all'][:L * R * 27].view(L, R, 27)

    def fused_rhs_diag(self, op, reg_weight=1.0, dense_from=None):
        """Right-hand side and Jacobi diagonal from ONE set-up sweep.  ``dense_from`` = c0 (factor form only): the sweep also leaves
        the rebuilt rows of the levels >= c0 in op['dense'] -- what the coarse-level block of the preconditioner is assembled from."""
        M = self.svh.num_unknowns
        b = torch.empty(M, dtype=torch.float32, device=self.device)
        diag = torch.empty(M, dtype=torch.float32, device=self.device)
        if dense_from is not None and op.get('row_format') == 'factors':
            self._arm_dense(op, int(dense_from))
        call('nksr_fused_rhs_diag', C.byref(op['op']), float(reg_weight), ptr(b), ptr(diag), stream())
        if op.get('dense') is not None:
            op['op'].dense_out = None          # (written; later sweeps must not write it again)
        return b, diag

    def _arm_dense(self, op, c0):
        L = self.svh.depth
        dense = torch.empty((L - c0, op['rows_total'], 27), dtype=torch.float32, device=self.device)
        op['dense'], op['dense_from'] = dense, c0
        op['op'].dense_from, op['op'].dense_out = c0, ptr(dense)
        return dense

    def _dense_coarse_rows(self, op, c0):
        """[L - c0, rows_total, 27] dense rows of the levels >= c0 of a factor-form operator (taken over: the operator forgets them)."""
        dense = op.get('dense')
        if dense is None or op.get('dense_from') != c0:
            dense = self._arm_dense(op, c0)
            call('nksr_fused_expand_rows', C.byref(op['op']), stream())
            op['op'].dense_out = None
        op['dense'] = None
        return dense

    def _small_field(self):
        """Single fields of at most 2^16 unknowns (configs[1], one scan of examples/recons_waymo_cpu.py): the policy takes the block of
        the levels >= 1 at once -- see solve_fused."""
        return 2 <= self.svh.depth < 5 and self.svh.num_unknowns <= SMALL_FIELD_UNKNOWNS      # (5+ levels: the block of the levels >= 2, as ever)

    def _pc_first_level(self, segments=None):
        """First level of the coarse-level block the solve is going to build at once, or None (see solve_fused / _coarse_precond)."""
        cfg = self.solver_config.get('coarse_precond')
        if cfg is False:
            return None
        auto = cfg is None and segments is None
        if auto and self.svh.depth < 5 and not self._small_field():
            return None
        cfg = cfg if isinstance(cfg, dict) else (dict(SMALL_FIELD_PC) if auto and self._small_field() else {})
        c0 = int(cfg.get('first_level', float(os.environ.get('NKSR_PC_LEVEL', 2))))
        off, M = self.svh.offsets, self.svh.num_unknowns
        return c0 if (0 < c0 < self.svh.depth and M - off[c0] >= 1) else None

    def stored_entries(self):
        """Non-zero entries of G and Q of the last matrix-free solve (counted by its diagonal pass; one small device read)."""
        t = getattr(self, '_stored_entries', None)
        return int(t.item()) if t is not None else None

    def fused_apply(self, op, x, reg_weight=1.0):
        """y = (w_p G^T G + w_n Q^T Q + reg I) x without the matrix (test / export helper)."""
        y = torch.empty_like(x)
        call('nksr_fused_apply', C.byref(op['op']), float(reg_weight), ptr(x.contiguous()), ptr(y), stream())
        return y

    def _coarse_precond(self, op, reg_weight, segments=None, sites=None, override=None):
        """Block preconditioner of the coarse levels (nksr_coarse_precond_t), or None -- coarse_precond.coarse_precond."""
        return coarse_precond.coarse_precond(self, op, reg_weight, segments, sites, override)

    def solve_fused(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight=1.0,
                    pos_sorted_keys=None, normal_sorted_keys=None, segments=None):
        """Matrix-free Jacobi-PCG on the normal equations: no assembly, ~8 bytes per dense kernel-row slot per
        iteration (examples/recons_waymo.py:33 ``fused_mode=True``).  Same system, same stopping rule as
        solve_non_fused; the iterates agree to fp32 rounding (different summation order)."""
        t0 = time.perf_counter()
        td = _tick('_', t0)
        op = self.fused_operator(pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, pos_sorted_keys, normal_sorted_keys,
                                 segments=segments)
        td = _tick('fused_operator', td)
        dev = self.device
        M = self.svh.num_unknowns
        b, diag = self.fused_rhs_diag(op, reg_weight, dense_from=self._pc_first_level(segments))
        td = _tick('rhs_diag', td)
        cfg, tol = self.solver_config, float(self.solver_config['tol'])
        max_iter, check_every = int(cfg['max_iter']), int(cfg['check_every'])
        # Preconditioner policy (coarse_precond = None): hierarchies of 5+ levels get the coarse-level block at once (Jacobi alone
        # needs ~47 iterations per tree_depth-5 chunk); shallower ones start with Jacobi -- the 1M-point headline converges in 11
        # iterations, a set-up would not pay -- and switch after one unconverged round of check_every iterations (sparse /
        # sensor-only inputs and adaptive_depth 2 take 100+ Jacobi iterations at depth 4 too).
        # Batched chunk solves (``segments``) always take the block at once: a restart decided on the joint residual would make a
        # chunk's iterates depend on its batch mates.
        # Small single fields (<= 2^16 unknowns; round 6): the block of the levels >= 1 at once, eight steps on [lmax / 40, lmax] -- the
        # block is a few thousand unknowns there and costs little, and one failed Jacobi round was most of the solve (configs[1] 39 ->
        # 18 iterations, the 10 000-point bunny scan 93 -> 53, the smoke sphere 94 -> 57: tools/small_pc_sweep.py).
        auto = cfg.get('coarse_precond') is None and segments is None
        small = auto and self._small_field()
        if small:
            # an iteration of such a field is 16 launches of a few microseconds: the 14 no-op iterations behind convergence at 18 of
            # a 16-iteration round cost as much as 5 real ones -- the host looks every 6 (same iterates: convergence is per iteration on the device)
            check_every = min(check_every, SMALL_FIELD_CHECK_EVERY)
        pc = self._coarse_precond(op, reg_weight, segments, override=SMALL_FIELD_PC if small else None) if (not auto or small or self.svh.depth >= 5) else None
        op['dense'] = None                      # (dense coarse rows nobody took over)
        td = _tick('coarse_precond', td)
        if cfg.get('verbose') or cfg.get('sync_timing'):
            torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        nseg = segments.nseg if segments is not None else 1
        pws = torch.empty(int(_lib.lib.nksr_pcg_vector_workspace_bytes_seg(M, nseg, self.svh.depth if segments is not None else 1)),
                          dtype=torch.uint8, device=dev)

        def pcg(rhs, rtol, iters, precond):
            sol = torch.empty(M, dtype=torch.float32, device=dev)
            inf = (C.c_double * 3)()
            call('nksr_pcg_solve_fused', C.byref(op['op']), float(reg_weight), ptr(diag), ptr(rhs), ptr(sol), float(rtol), int(iters),
                 check_every, ptr(pws), C.byref(precond['pc']) if precond else None, C.byref(segments.c) if segments is not None else None,
                 inf, stream())
            # a segment whose Chebyshev block lost definiteness (r.z <= 0: eigenvalue bound too small) restarts with Jacobi alone on
            # the device (csrc/pcg.hip: k_spcg_pupdate) -- counted, not raised; only r.z <= 0 with Jacobi itself / NaN is an error
            fallbacks[0] += int(inf[2])
            if inf[1] < 0:
                raise RuntimeError('PCG breakdown (r.z <= 0 with the Jacobi preconditioner after %d iterations, relative residual %.3e): '
                                   'the system is not positive definite (non-finite rows or weights?)' % (int(inf[0]), -inf[1]))
            return sol, int(inf[0]), float(inf[1])
        fallbacks = [0]
        if pc is not None or not auto or max_iter <= check_every:
            x, iters, rel = pcg(b, tol, max_iter, pc)
        else:
            x, iters, rel = pcg(b, tol, check_every, None)
            if rel > tol:
                # restart on the residual with the block preconditioner: A e = b - A x to the remaining accuracy
                pc = self._coarse_precond(op, reg_weight)
                r = b - self.fused_apply(op, x, reg_weight)
                bn, rn = float(torch.linalg.vector_norm(b.double())), float(torch.linalg.vector_norm(r.double()))
                if rn > tol * bn:
                    e, it2, rel2 = pcg(r, tol * bn / rn, max_iter - iters, pc)
                    x, iters, rel = x + e, iters + it2, rel2 * rn / bn
                else:
                    rel = rn / bn
        info = (float(iters), rel)
        t2 = time.perf_counter()
        if fallbacks[0]:
            import warnings
            warnings.warn('%d segment(s) of the solve restarted with the Jacobi preconditioner alone (the coarse-level block lost '
                          'definiteness: eigenvalue bound too small); the result is valid, the iteration count is higher' % fallbacks[0])
        self.alpha = x
        self.matrix = None
        self._fused_op, self._fused_reg = op, float(reg_weight)
        self._pc = pc if segments is None else None      # (a batched solve's block needs its segments: not kept)
        self._stored_entries = op['nnz_counter']
        self.rhs, self.diag = b, diag
        self.nnz = 0
        self.solve_info = {'iters': int(info[0]), 'rel_residual': float(info[1]), 'M': int(M), 'nnz': 0, 'fused': True,
                           'kernel_row_slots': 27 * self.svh.depth * op['rows_total'], 'partial_blocks': op['nblocks'],
                           'coarse_precond': ({k: pc[k] for k in ('first_level', 'unknowns', 'nnz', 'steps', 'lambda', 'gershgorin')} if pc else None),
                           'segments': nseg, 'segment_info': segments.info if segments is not None else None,
                           'jacobi_fallbacks': fallbacks[0], 't_assemble': t1 - t0, 't_pcg': t2 - t1}
        if self.solver_config.get('verbose'):
            print('[KernelField] fused: M=%d rows=%d iters=%d rel=%.3e rows+rhs=%.3fs pcg=%.3fs' % (
                M, op['rows_total'], int(info[0]), float(info[1]), t1 - t0, t2 - t1))
        if not self._wants_grad(normal_value):
            self._fused_op = self._pc = None          # only the backward pass needs the operator again: do not pin ~2 GB of rows
        self._attach_autograd(pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight)
        return self

    # ---- differentiable solve (training path, models/nksr_net.py:105-112) ---------------------------------------
    def _solve_system(self, rhs):
        """A^-1 rhs with the system of the last solve (assembled CSR or matrix-free operator), same tolerance, same
        preconditioner (the coarse-level block of the forward solve, when it had one)."""
        from .. import solver
        cfg = self.solver_config
        pc = getattr(self, '_pc', None)
        if self.matrix is not None:
            rowptr, cols, vals, diag = self.matrix
            return solver.pcg_solve(rowptr, cols, vals, diag, rhs.contiguous(), tol=cfg['tol'], max_iter=cfg['max_iter'], check_every=cfg['check_every'],
                                    precond=pc['pc'] if pc else None)[0]
        if getattr(self, '_fused_op', None) is None:
            raise RuntimeError('the system of the last solve is gone: call solve*() under torch.enable_grad() with normal_value.requires_grad')
        M = self.svh.num_unknowns
        x = torch.empty(M, dtype=torch.float32, device=self.device)
        pws = torch.empty(int(_lib.lib.nksr_pcg_vector_workspace_bytes(M)), dtype=torch.uint8, device=self.device)
        info = (C.c_double * 3)()
        call('nksr_pcg_solve_fused', C.byref(self._fused_op['op']), self._fused_reg, ptr(self.diag), ptr(rhs.contiguous()), ptr(x), float(cfg['tol']),
             int(cfg['max_iter']), int(cfg['check_every']), ptr(pws), C.byref(pc['pc']) if pc else None, None, info, stream())
        if info[1] < 0:
            raise RuntimeError('PCG breakdown in the adjoint solve (r.z <= 0 with the Jacobi preconditioner): the system is not positive definite')
        return x

    def _theta(self):
        """The caller's basis-feature tensors and interpolator parameters that take part in an autograd graph.  The switch is the
        FEATURES: a field whose basis features carry no graph (inference: they come out of the HIP U-Net; tests: constants) stays
        out of autograd in theta even though an nn.Module's parameters require grad by default."""
        th = [f for f in self._feat_in if torch.is_tensor(f) and f.requires_grad]
        if not th:
            return []
        for m in self._interps_in:
            if isinstance(m, torch.nn.Module):
                th += [q for q in m.parameters() if q.requires_grad]
        return th

    def _wants_grad(self, normal_value):
        return torch.is_grad_enabled() and ((torch.is_tensor(normal_value) and normal_value.requires_grad) or len(self._theta()) > 0)

    def _attach_autograd(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight):
        """Under autograd, alpha becomes a differentiable function of the normal targets, the basis features and the interpolator
        weights by implicit differentiation: one more PCG solve with the same system in backward, then (for the features /
        weights) the vector-Jacobian product through the torch statement of the kernel rows (fields/kernel_rows_torch.py)."""
        if not self._wants_grad(normal_value):
            return
        nv = normal_value if torch.is_tensor(normal_value) else torch.zeros((0, 3), device=self.device)
        self.alpha = _SolveFunction.apply(self, self.alpha, None if pos_xyz is None else pos_xyz.detach(),
                                          None if normal_xyz is None else normal_xyz.detach(), nv, float(pos_weight), float(normal_weight),
                                          *self._theta())

    def _theta_vjp(self, sets, alpha, lam=None):
        """sum_r g_r . dR'_r / dtheta over the site sets ``sets`` -- autograd.theta_vjp."""
        return autograd.theta_vjp(self, sets, alpha, lam)

    def solve(self, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight=1.0, fused_mode=True,
              pos_sorted_keys=None, normal_sorted_keys=None, segments=None):
        """``fused_mode=True`` (the reference's memory-lean operator, examples/recons_waymo.py:33): matrix-free solve,
        no assembly; ``False``: assemble the CSR and stream it (solve_non_fused -- the path the training code needs,
        models/nksr_net.py:105-112).  DESIGN.md section 3.5 has the cost model of the two."""
        if fused_mode:
            return self.solve_fused(pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight,
                                    pos_sorted_keys, normal_sorted_keys, segments=segments)
        if segments is not None and segments.nseg > 1:
            raise RuntimeError('batched chunk solves run through the matrix-free solve (fused_mode=True)')
        return self.solve_non_fused(pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight,
                                    pos_sorted_keys, normal_sorted_keys)

    # ---- evaluation -------------------------------------------------------------------------------------
    def _evaluate_f_model(self, xyz, grad, max_points=1 << 22):
        if torch.is_grad_enabled() and (self.alpha.requires_grad or self._theta()):
            f, g = _EvaluateFunction.apply(self, self.alpha, xyz.detach(), bool(grad), max_points, *self._theta())
            return EvaluationResult(f, g if grad else None)
        return self._evaluate_raw(self.alpha, xyz, grad, max_points)

    def _alpha_hier(self, alpha):
        """A copy of the hierarchy whose psi arrays hold alpha_j psi_j: evaluation then gathers ONE 16-byte value per neighbour
        (these per-point kernels are bound by the number of gather instructions).  Rebuilt when alpha changes."""
        key = (alpha.data_ptr(), alpha._version, str(self.device))
        if self._apsi_key != key:
            off = self.svh.offsets
            self._apsi = [(self._psi[d] * alpha[off[d]:off[d] + self._psi[d].shape[0], None]).contiguous() for d in range(self.svh.depth)]
            h = HierT.from_buffer_copy(self._hier)
            for d in range(self.svh.depth):
                h.lv[d].psi = ptr(self._apsi[d])
            self._apsi_hier, self._apsi_key = h, key
        return self._apsi_hier

    def _evaluate_raw(self, alpha, xyz, grad, max_points=1 << 22, active_only=False):
        n = xyz.shape[0]
        xyz = xyz.to(self.device)
        alpha = alpha.detach().contiguous()
        if alpha is self.alpha or alpha.data_ptr() == self.alpha.data_ptr():
            hier, alpha_arg = self._alpha_hier(alpha), None
        else:
            hier, alpha_arg = self._hier, alpha
        f = torch.empty(n, dtype=torch.float32, device=self.device)
        g = torch.empty((n, 3), dtype=torch.float32, device=self.device) if grad else None
        for s in range(0, n, max_points):
            e = min(n, s + max_points)
            xs = xyz[s:e].contiguous()
            fs = f[s:e]
            gs = g[s:e] if grad else None
            call('nksr_evaluate_f', C.byref(hier), ptr(alpha_arg), ptr(xs), e - s, int(self.approx_kernel_grad), int(bool(active_only)),
                 ptr(fs), ptr(gs), stream())
        return EvaluationResult(f, g)

    def to_(self, device):
        device = torch.device(device)
        self.svh.to_(device)
        self._feat = [t.to(device) for t in self._feat]
        self._psi = [t.to(device) for t in self._psi]
        self._mlp = [t.to(device) for t in self._mlp]
        self.alpha = self.alpha.to(device)           # (the setter drops the evaluation cache: it points into the old arrays)
        self.matrix = None
        self._fused_op = self._pc = None
        if device.type == 'cuda':
            self._hier = self._make_hier()
        if self.mask_field is not None:
            self.mask_field.to_(device)
        return self


class _PackedInterpolator:
    """Interpolator stand-in carrying only the packed weights (used when a field is re-created from
    a payload: serialisation, chunk exchange)."""

    def __init__(self, kernel_dim, hidden_dim, packed):
        self.kernel_dim, self.hidden_dim, self._packed = int(kernel_dim), int(hidden_dim), packed

    def packed(self):
        return self._packed


def save_field(field, path):
    """Serialise a solved KernelField (hierarchy keys, basis features, alpha, interpolator weights,
    global scale).  SURVEY.md section 8(f)-3: the reference has no on-disk format for solved fields;
    this enables spill-to-disk of chunks and checkpointing."""
    from ..chunking import pack_field
    ints, flts = pack_field(field)
    torch.save({'format': 'nksr_amd.KernelField.v2', 'adaptive_depth': int(getattr(field.mask_field, 'adaptive_depth', 1)), 'ints': ints.cpu(), 'flts': flts.cpu(), 'voxel_size': field.svh.voxel_size,
                'hidden': field.hidden, 'kdim': field.kdim, 'scale': field.scale, 'mlp': [m.cpu() for m in field._mlp],
                'solve_info': field.solve_info}, path)


def load_field(path, device):
    from ..chunking import unpack_field
    from .mask_fields import LayerField
    st = torch.load(path, map_location='cpu')
    if st.get('format') != 'nksr_amd.KernelField.v2':
        raise RuntimeError('%s is not a serialised KernelField' % path)
    interps = [_PackedInterpolator(st['kdim'], st['hidden'], m) for m in st['mlp']]
    fld = unpack_field(st['ints'], st['flts'], st['voxel_size'], interps, torch.device(device))
    fld.set_scale(st['scale'])
    fld.solve_info = st.get('solve_info', {})
    if fld.mask_field is None:          # a UDF (NeuralField) mask travels inside the payload
        fld.set_mask_field(LayerField(fld.svh, st.get('adaptive_depth', 1)))
    return fld
