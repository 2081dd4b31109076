"""The coarse-level block preconditioner (csrc/cheb.hip, k_cheb_coeffs .. cheb_apply, the packer, the eigenvalue bounds) against the
fp64 references of tests/coarse_precond_ref.py, which tests/test_coarse_precond_cpu.py verifies without a GPU.

The margin rule.  An fp32 evaluation of the operator cannot sit closer to the closed form than rounding allows; how close that is
for a given input is measured, not guessed: the same recurrence in numpy fp32 (R.rounding_floor, never below 2^-24).  The GPU sums a
row on a tree over 64 or 16 lanes and fuses some multiply-adds where numpy sums left to right: 8 x that floor covers another order
of the same roundings (floors are 6e-8 .. 5.4e-7, so bounds are 4.8e-7 .. 4.3e-6) and admits no mistake of the kind this file is
for -- a coefficient one step off, a forgotten unit diagonal, a column of the wrong segment are errors of 1e-3 .. 1.  Every check
prints the measured value beside its bound (parity_util.check).

`lambda` and `gersh` are always passed explicitly, so the interval is the test's and not the power iteration's."""
import ctypes as C

import numpy as np
import pytest
import torch

import coarse_precond_ref as R
import parity_util as pu
import spmv_layout

pytestmark = pytest.mark.gpu

FORMATS = [(0, 0.0), (1, 0.0), (1, R.DROP)]
IDS = ['plain', 'packed-drop0', 'packed-drop']
MARGIN = 8.0


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


class Precond:
    """A CoarsePrecondT built by hand from numpy arrays (blk: a block of the reference; pk: its pack_ref, or None for format 0)."""

    def __init__(self, blk, pk, lam, steps, gersh=None, scale=R.SCALE, ratio=R.RATIO, first=0, with_row_seg=True):
        from nksr_amd import _lib
        n, self.nseg = blk['n'], len(lam)
        self.n = n
        pc = _lib.CoarsePrecondT()
        pc.first, pc.n, pc.steps, pc.lambda_scale, pc.ratio = first, n, steps, scale, ratio
        k = self.keep = dict(lam=_dev(lam, np.float32), coef=torch.full((self.nseg * R.STRIDE,), float('nan'), device='cuda'))
        pc.lambda_, pc.coef = k['lam'].data_ptr(), k['coef'].data_ptr()
        if gersh is not None:
            k['gersh'] = _dev(gersh, np.float32)
            pc.gersh = k['gersh'].data_ptr()
        # the work arrays start as NaN: whatever a step reads before the kernels wrote it shows in z
        k['work'] = torch.full(((4 if pk is not None else 3) * n,), float('nan'), device='cuda')
        pc.work = k['work'].data_ptr()
        if pk is None:
            pc.format = 0
            k.update(rowptr=_dev(blk['rowptr'], np.int32), cols=_dev(blk['cols'], np.int32), vals=_dev(blk['vals'], np.float32),
                     diag=_dev(blk['diag'], np.float32))
            pc.rowptr, pc.cols, pc.vals, pc.diag = (k[f].data_ptr() for f in ('rowptr', 'cols', 'vals', 'diag'))
            if with_row_seg:
                k['row_seg'] = _dev(blk['row_seg'], np.int32)
                pc.row_seg = k['row_seg'].data_ptr()
        else:
            pc.format = 1
            packed = pk['packed'] if len(pk['packed']) else np.zeros(1, np.uint32)
            k.update(packed=_dev(packed.view(np.int32), np.int32), prow=_dev(pk['packed_rowptr'], np.int32), dis=_dev(pk['dis'], np.float32),
                     o2n=_dev(pk['old_of_new'], np.int32), seg_base=_dev(pk['seg_base'], np.int32), row_seg=_dev(pk['row_seg_new'], np.int32))
            pc.packed, pc.packed_rowptr, pc.dis, pc.old_of_new, pc.seg_base, pc.row_seg = (
                k[f].data_ptr() for f in ('packed', 'prow', 'dis', 'o2n', 'seg_base', 'row_seg'))
        self.pc = pc

    def apply(self, r):
        from nksr_amd._lib import call, stream
        rd = _dev(r, np.float32)
        z = torch.full((self.n,), float('nan'), device='cuda')
        call('nksr_coarse_precond_apply', C.byref(self.pc), self.nseg, rd.data_ptr(), z.data_ptr(), stream())
        return z.cpu().numpy()


def _precond(prep, steps, lam=None, **kw):
    return Precond(prep['blk'], prep['pk'], prep['lam'] if lam is None else lam, steps, **kw)


def test_drop_tolerance_is_the_projects():
    from nksr_amd.fields import coarse_precond as cp
    from nksr_amd import _lib
    assert cp.PC_DROP_TOL == R.DROP and cp.PC_RATIO == R.RATIO and _lib.PC_MAX_STEPS == R.MAX_STEPS


# ---- 1, 2: the operator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,drop', FORMATS, ids=IDS)
@pytest.mark.parametrize('name', list(R.BLOCKS))
def test_operator_matches_the_closed_form(name, fmt, drop):
    """z of nksr_coarse_precond_apply against the eigen-decomposition formula -- on S for the plain block, on the half-rounded and
    dropped S_h that the packed words denote for the packed one (half precision is in the operator, not in the tolerance) -- as max-abs
    error over max |z_ref|, worst segment; steps 1 (init and the `last` step that writes z, one launch each) .. 16.
    CPU floor (fp32 recurrence in numpy): 6.0e-8 .. 5.4e-7 over the 120 cases, so bounds 4.8e-7 .. 4.3e-6.  Measured on MI355X:
    plain 1.0e-8 .. 5.2e-7 (at most 0.25 of its bound), packed without drop 1.3e-9 .. 2.9e-7 (0.32), packed with the drop
    1.3e-9 .. 2.5e-7 (0.16)."""
    prep = R.prepared(name, fmt, drop)
    blk = prep['blk']
    r = R.rhs(blk['n'])
    for steps in R.STEPS:
        zref, floor = R.rounding_floor(prep, r, steps)
        z = _precond(prep, steps, with_row_seg=blk['nseg'] > 1).apply(r)
        assert np.isfinite(z).all()
        pu.report('coarse_precond:floor:%s:%s:steps%d' % (name, IDS[FORMATS.index((fmt, drop))], steps), cpu_fp32_floor=floor)
        pu.check('coarse_precond:operator:%s:%s:steps%d' % (name, IDS[FORMATS.index((fmt, drop))], steps), R.rel_err(z, zref, blk['row_seg']), MARGIN * floor)      # floor / GPU: see the docstring


# ---- 3: the packer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('drop', [0.0, R.DROP], ids=['drop0', 'drop'])
@pytest.mark.parametrize('name', list(R.BLOCKS))
def test_packer_is_exact(name, drop):
    """nksr_coarse_pack_count / nksr_coarse_pack through the project's own _pack_block against pack_ref: lengths, kept pattern, column
    halves, value halves and D^-1/2 all bitwise (no fast-math: 1 / sqrt, the products and the rounding to half are correctly rounded on
    both sides), and the packed block is bitwise symmetric."""
    from nksr_amd.fields.coarse_precond import _pack_block
    blk = R.block(name)
    ref = R.prepared(name, 1, drop)['pk']
    rs = _dev(blk['row_seg'], np.int32)
    counts = torch.bincount(rs.long(), minlength=blk['nseg'])
    packed, prow, dis, o2n, seg_base, row_seg_new, kept = _pack_block(_dev(blk['rowptr'], np.int32), _dev(blk['cols'], np.int32), _dev(blk['vals'], np.float32),
                                                                      _dev(blk['diag'], np.float32), blk['n'], rs, counts, drop)
    prow, o2n = prow.cpu().numpy(), o2n.cpu().numpy()
    assert np.array_equal(np.diff(prow), ref['lens']) and prow[0] == 0 and kept == len(ref['packed'])
    assert np.array_equal(o2n, ref['old_of_new']) and np.array_equal(seg_base.cpu().numpy(), ref['seg_base'])
    assert np.array_equal(row_seg_new.cpu().numpy(), ref['row_seg_new'])
    words = packed.cpu().numpy().view(np.uint32)[:kept]
    assert np.array_equal(words & 0xFFFF, ref['packed'] & 0xFFFF), 'column halves / kept pattern differ'
    dv = (words >> 16).astype(np.int64) - (ref['packed'] >> 16).astype(np.int64)
    pu.report('coarse_precond:packer:%s:drop%g' % (name, drop), kept=kept, value_halves_differing=int((dv != 0).sum()))
    assert not dv.any(), 'value halves differ in %d entries (by at most %d half ulps)' % ((dv != 0).sum(), np.abs(dv).max())
    assert np.array_equal(dis.cpu().numpy().view(np.uint32), ref['dis'].view(np.uint32))
    # bitwise symmetry, from the GPU's words alone: (i, j) kept with bits h  <=>  (j, i) kept with bits h
    rows_new = np.repeat(np.arange(blk['n']), np.diff(prow))
    cols_new = (words & 0xFFFF).astype(np.int64) + ref['seg_base'][ref['row_seg_new'][rows_new]]
    fwd = dict(zip(zip(rows_new.tolist(), cols_new.tolist()), (words >> 16).tolist()))
    assert len(fwd) == kept and all(fwd.get((j, i)) == h for (i, j), h in fwd.items())


# ---- 4: degenerate and capped intervals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,drop', [(0, 0.0), (1, R.DROP)], ids=['plain', 'packed-drop'])
def test_degenerate_and_capped_intervals(fmt, drop):
    prep = R.prepared('n1501x3', fmt, drop)
    blk = prep['blk']
    r = R.rhs(blk['n'], 4)
    steps = 8
    base = _precond(prep, steps).apply(r)
    D = blk['diag'].astype(np.float64)
    # one division (plain) is within 2^-24 = u; the packed form computes fl(fl(r dis) dis) with dis = fl(1 / fl(sqrt D)), 2 u off at the
    # worst, entering twice, and rounds two products: (2 x 2 + 2) u, first order
    jacobi_bound = (1.0 if fmt == 0 else 6.0) * R.U32
    for c in (0, 2):
        m = blk['row_seg'] == c
        for bad in (0.0, -1.0, np.inf, np.nan):
            lam = prep['lam'].copy()
            lam[c] = bad
            z = _precond(prep, steps, lam=lam).apply(r)
            pu.check('coarse_precond:degenerate:%s:seg%d:lambda=%s' % (IDS[FORMATS.index((fmt, drop))], c, bad),
                     np.abs(z[m] * D[m] / r[m].astype(np.float64) - 1.0).max(), jacobi_bound)           # MI355X: plain 5.5e-8 .. 5.7e-8 of 6.0e-8, packed <= 2.3e-7 of 3.6e-7
            assert np.array_equal(z[~m].view(np.uint32), base[~m].view(np.uint32)), 'the other segments changed'
    # a Gershgorin bound below lambda_scale * lambda moves the interval: closed form on the capped top
    gersh = (prep['lam'].astype(np.float64) * np.array([0.9, 2.0, 1.05])).astype(np.float32)
    assert (R.interval_top(prep['lam'], gersh, R.SCALE) == np.where([True, False, True], gersh.astype(np.float64), np.float64(np.float32(R.SCALE)) * prep['lam'])).all()
    zref, floor = R.rounding_floor(prep, r, steps, gersh=gersh)
    z = _precond(prep, steps, gersh=gersh).apply(r)
    # CPU floor 1.4e-7 (plain) / 1.4e-7 (packed); MI355X 1.9e-7 / 1.2e-7, the same with the infinite estimate below
    pu.check('coarse_precond:capped:%s' % IDS[FORMATS.index((fmt, drop))], R.rel_err(z, zref, blk['row_seg']), MARGIN * floor)
    assert R.rel_err(base, zref, blk['row_seg']) > 100 * MARGIN * floor          # (and the cap does matter on this input)
    # an infinite estimate under a cap takes the cap; lambda <= 0 / NaN stay degenerate under it (covered by the table test on the CPU)
    lam = prep['lam'].copy()
    lam[0] = np.inf
    zref, floor = R.rounding_floor(prep, r, steps, lam=lam, gersh=gersh)
    pu.check('coarse_precond:capped_inf:%s' % IDS[FORMATS.index((fmt, drop))],
             R.rel_err(_precond(prep, steps, lam=lam, gersh=gersh).apply(r), zref, blk['row_seg']), MARGIN * floor)
    # no bound and a bound above the estimate: the same bits
    z_big = _precond(prep, steps, gersh=prep['lam'] * np.float32(3.0)).apply(r)
    assert np.array_equal(z_big.view(np.uint32), base.view(np.uint32))


# ---- 5: symmetry and definiteness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,drop', FORMATS, ids=IDS)
def test_operator_is_symmetric_and_positive_and_loses_definiteness_with_a_quarter_interval(fmt, drop):
    prep = R.prepared('n1501x3', fmt, drop)
    blk = prep['blk']
    n = blk['n']
    tag = IDS[FORMATS.index((fmt, drop))]
    for steps in (8, 10):
        P = _precond(prep, steps)
        u, v = R.rhs(n, 50), R.rhs(n, 51)
        Pu, Pv = P.apply(u).astype(np.float64), P.apply(v).astype(np.float64)
        Pu32, Pv32 = (R.reference(prep, x, steps, dtype=np.float32).astype(np.float64) for x in (u, v))
        norm = np.linalg.norm(u) * np.linalg.norm(R.reference(prep, v, steps))
        floor = max(abs(u.astype(np.float64) @ Pv32 - v.astype(np.float64) @ Pu32) / norm, R.U32)
        pu.report('coarse_precond:symmetry_floor:%s:steps%d' % (tag, steps), cpu_fp32_floor=floor)
        # CPU floor: 2^-24 in all six cases (the fp32 recurrence is symmetric to better than that); MI355X 6.0e-11 .. 2.7e-9
        pu.check('coarse_precond:symmetry:%s:steps%d' % (tag, steps), abs(u.astype(np.float64) @ Pv - v.astype(np.float64) @ Pu) / norm, MARGIN * floor)
        assert v.astype(np.float64) @ Pv > 0 and u.astype(np.float64) @ Pu > 0
    # lambda_scale = 0.25: the reference's p turns negative; for the eigenvector where it is most negative so does the GPU's v.P v
    steps = 8
    top = R.interval_top(prep['lam'], None, 0.25)
    rows, w, U = prep['eigs'][0]
    p = R.poly(w, top[0], R.RATIO, steps)
    k = int(np.argmin(p))
    assert p[k] < 0
    v = np.zeros(n)
    v[rows] = U[:, k] / prep['dis'][rows]                  # D^-1/2 v is the eigenvector: v.P v = p(lambda_k)
    v32 = v.astype(np.float32)
    z = _precond(prep, steps, scale=0.25).apply(v32).astype(np.float64)
    quad, want = float(v32.astype(np.float64) @ z), float(v32.astype(np.float64) @ R.reference(prep, v32, steps, scale=0.25))
    pu.report('coarse_precond:indefinite:%s' % tag, p_min=float(p[k]), vPv_gpu=quad, vPv_ref=want)
    assert want < 0 and quad < 0


# ---- 6: independence of the batch mates -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,drop', FORMATS, ids=IDS)
@pytest.mark.parametrize('name', ['n65x3', 'n1501x3'])
def test_a_segment_does_not_depend_on_its_batch_mates(name, fmt, drop):
    prep = R.prepared(name, fmt, drop)
    blk = prep['blk']
    r = R.rhs(blk['n'], 6)
    for steps in (1, 10):
        P = _precond(prep, steps)
        z = P.apply(r)
        assert np.array_equal(P.apply(r).view(np.uint32), z.view(np.uint32)), 'two identical calls differ'
        for c in range(blk['nseg']):
            sub, rows = R.sub_block(blk, c)
            pk = R.pack_ref(sub['rowptr'], sub['cols'], sub['vals'], sub['diag'], None, drop) if fmt else None
            alone = Precond(sub, pk, prep['lam'][c:c + 1], steps, with_row_seg=False).apply(r[rows])
            assert np.array_equal(alone.view(np.uint32), z[rows].view(np.uint32)), 'segment %d alone differs from segment %d in the batch' % (c, c)
            other = r.copy()
            other[blk['row_seg'] == (c + 1) % blk['nseg']] = np.nan
            zn = P.apply(other)
            assert np.array_equal(zn[rows].view(np.uint32), z[rows].view(np.uint32)), 'NaN of another segment reached segment %d' % c
            assert np.isnan(zn[blk['row_seg'] == (c + 1) % blk['nseg']]).all()


# ---- 7: eigenvalue bounds ---------------------------------------------------------------------------------------------------------
def _bound_check(name, got, ref64, ref32):
    got, ref64, ref32 = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, ref64, ref32))
    nz = ref64 != 0
    assert (got[~nz] == 0).all()
    floor = max(float(np.abs(ref32[nz] / ref64[nz] - 1).max()), R.U32)
    pu.report(name + ':floor', cpu_fp32_floor=floor)
    # CPU floors 6.0e-8 .. 6.9e-8; MI355X: power estimates 1.4e-9 .. 3.9e-8, Gershgorin 0 .. 7.4e-8
    pu.check(name, np.abs(got[nz] / ref64[nz] - 1).max(), MARGIN * floor)


def test_eigenvalue_bounds():
    """nksr_coarse_lambda_max (without and with segments), nksr_coarse_lambda_max_packed, nksr_coarse_gershgorin (both formats, 1 and 3
    segments) against power_ref / gersh_ref in fp64; the floor is the same restatement in fp32.  And the order that makes the scheme
    sound: estimate <= lambda_max <= Gershgorin against eigvalsh."""
    from nksr_amd import _lib
    from nksr_amd._lib import call, stream
    iters = 8
    for name in R.BOUND_BLOCKS:
        for fmt, drop in FORMATS:
            prep = R.prepared(name, fmt, drop)
            blk, pk = prep['blk'], prep['pk']
            n, nseg = blk['n'], blk['nseg']
            tag = '%s:%s' % (name, IDS[FORMATS.index((fmt, drop))])
            true = R.lambda_true(prep['S'], blk['row_seg'])
            P = _precond(prep, 8)
            work = torch.full((2 * n,), float('nan'), device='cuda')
            lam = torch.full((nseg,), float('nan'), device='cuda')
            if fmt == 1:
                call('nksr_coarse_lambda_max_packed', C.byref(P.pc), nseg, iters, work.data_ptr(), lam.data_ptr(), stream())
                _bound_check('coarse_precond:lambda_packed:' + tag, lam.cpu().numpy(), R.power_packed(pk, iters), R.power_packed(pk, iters, np.float32))
                g64, g32 = R.gersh_ref(pk=pk), R.gersh_ref(pk=pk, dtype=np.float32)
            else:
                k = P.keep
                if name == 'ranges':          # segments as ranges behind `first` finer unknowns; segment 3 has no coarse row
                    _, first, lo, hi = R.ranges_block()
                    seg = _lib.SegmentsT()
                    lo_d, hi_d = _dev(lo, np.int32), _dev(hi, np.int32)
                    seg.nseg, seg.nranges, seg.lo, seg.hi = 4, 3, lo_d.data_ptr(), hi_d.data_ptr()
                    lam4 = torch.full((4,), float('nan'), device='cuda')
                    call('nksr_coarse_lambda_max', k['rowptr'].data_ptr(), k['cols'].data_ptr(), k['vals'].data_ptr(), k['diag'].data_ptr(), n, iters,
                         work.data_ptr(), lam4.data_ptr(), C.byref(seg), first, stream())
                    assert float(lam4[3]) == 0.0
                    lam = lam4[:3]
                    _bound_check('coarse_precond:lambda_segments:' + tag, lam.cpu().numpy(), R.power_plain(blk, iters, row_seg=blk['row_seg']),
                                 R.power_plain(blk, iters, np.float32, row_seg=blk['row_seg']))
                else:                         # without segments: one ratio over the whole block -- of a block-diagonal matrix too
                    lam1 = torch.full((1,), float('nan'), device='cuda')
                    call('nksr_coarse_lambda_max', k['rowptr'].data_ptr(), k['cols'].data_ptr(), k['vals'].data_ptr(), k['diag'].data_ptr(), n, iters,
                         work.data_ptr(), lam1.data_ptr(), None, 0, stream())
                    _bound_check('coarse_precond:lambda_whole:' + tag, lam1.cpu().numpy(), R.power_plain(blk, iters), R.power_plain(blk, iters, np.float32))
                    lam = lam1.expand(nseg) if nseg > 1 else lam1
                    true_whole = true.max()
                    assert float(lam1) <= true_whole * (1 + 1e-5)
                g64, g32 = R.gersh_ref(blk=blk, row_seg=blk['row_seg']), R.gersh_ref(blk=blk, row_seg=blk['row_seg'], dtype=np.float32)
            gersh = torch.full((nseg,), float('nan'), device='cuda')
            call('nksr_coarse_gershgorin', C.byref(P.pc), nseg, work.data_ptr(), gersh.data_ptr(), stream())
            _bound_check('coarse_precond:gershgorin:' + tag, gersh.cpu().numpy(), g64, g32)
            lam_h, gersh_h = lam.cpu().numpy().astype(np.float64), gersh.cpu().numpy().astype(np.float64)
            if not (fmt == 0 and name != 'ranges' and nseg > 1):      # (a whole-block estimate says nothing about the single segments)
                assert (lam_h <= true * (1 + 1e-5)).all(), (tag, lam_h, true)
            assert (true <= gersh_h * (1 + 1e-5)).all(), (tag, true, gersh_h)
            if fmt == 0 and nseg > 1:           # one segment asked of a block that holds three: the largest of the three bounds
                g1 = torch.full((1,), float('nan'), device='cuda')
                call('nksr_coarse_gershgorin', C.byref(P.pc), 1, work.data_ptr(), g1.data_ptr(), stream())
                assert float(g1) == float(gersh.max())


# ---- 8: through the solve ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,drop', [(0, 0.0), (1, R.DROP)], ids=['plain', 'packed-drop'])
def test_first_pcg_iterate_carries_the_preconditioner(fmt, drop):
    """An SPD system whose last n unknowns are the block (first > 0), in the streaming SpMV's col_format-0 tile layout; one iteration
    from x0 = 0 returns x1 = alpha z0 with z0 = [b_f / D_f ; P b_c], alpha = b.z0 / z0.A z0: the `first` offset and the r.z wiring of
    the solve, which the direct entry point bypasses."""
    from nksr_amd import solver
    M, n = 700, 257
    first = M - n
    full = R.make_block(np.zeros(M, np.int32), 31)
    rng = np.random.default_rng(32)
    dense_c = full['dense'][first:, first:].astype(np.float32)
    rowptr_c, cols_c, vals_c = R.csr_diag_last(dense_c, rng)
    blk = dict(rowptr=rowptr_c, cols=cols_c, vals=vals_c, diag=full['diag'][first:].copy(), n=n, nseg=1, row_seg=np.zeros(n, np.int32),
               dense=dense_c.astype(np.float64))
    pk = R.pack_ref(rowptr_c, cols_c, vals_c, blk['diag'], None, drop) if fmt else None
    if fmt:
        S, dis = pk['S_h'], pk['dis_old'].astype(np.float64)
    else:
        S, dis = R.scaled_dense(blk)
    eigs = R.eig_segments(S, blk['row_seg'])
    prep = dict(blk=blk, pk=pk, S=S, dis=dis, eigs=eigs, lam=np.array([eigs[0][1][-1]], np.float32))
    steps = 8
    b = R.rhs(M, 8)
    # the whole matrix in the tile layout (the encoder of test_csr_physical_layouts_roundtrip_on_cpu)
    c0, v0 = spmv_layout.encode0(full['cols'], full['vals'])
    P = Precond(blk, pk, prep['lam'], steps, first=first, with_row_seg=False)
    x, iters, _ = solver.pcg_solve(_dev(full['rowptr'], np.int32), _dev(c0, np.int32), _dev(v0, np.float32), _dev(full['diag'], np.float32), _dev(b, np.float32),
                                   tol=0.0, max_iter=1, check_every=1, precond=P.pc)
    assert iters == 1 and solver.last_fallbacks == 0
    x = x.cpu().numpy()

    def x1(zc, f):
        z0 = np.concatenate([(b[:first].astype(f) / full['diag'][:first].astype(f)), zc.astype(f)]).astype(f)
        Az = R._rowsum(full['rowptr'], full['vals'].astype(f) * z0[full['cols']])
        alpha = f((b.astype(np.float64) @ z0.astype(np.float64)) / (z0.astype(np.float64) @ Az.astype(np.float64)))
        return (alpha * z0).astype(f)
    ref = x1(R.reference(prep, b[first:], steps), np.float64)
    r32 = x1(R.reference(prep, b[first:], steps, dtype=np.float32), np.float32)
    seg = np.concatenate([np.zeros(first, np.int64), np.ones(n, np.int64)])          # the fine and the coarse slice, each over its own max
    floor = max(R.rel_err(r32, ref, seg), R.U32)
    pu.report('coarse_precond:solve_floor:%s' % IDS[FORMATS.index((fmt, drop))], cpu_fp32_floor=floor)
    # CPU floor 8.7e-8 (plain) / 1.8e-7 (packed); MI355X 8.5e-8 / 9.2e-8
    pu.check('coarse_precond:first_iterate:%s' % IDS[FORMATS.index((fmt, drop))], R.rel_err(x, ref, seg), MARGIN * floor)
