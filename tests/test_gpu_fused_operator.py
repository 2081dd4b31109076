"""The matrix-free operator (csrc/fused_tables.hip, fused_sweep.hip, fused.hip) by itself, one crafted row layout at a time (tests/fused_op_ref.py: what each layout
is for; tests/test_fused_op_ref_cpu.py asserts that it has that property):

  * its tables word for word against tables_ref, a restatement of what span / item_begin / counts / nbr32 / nbrT MEAN;
  * nksr_fused_apply and nksr_fused_rhs_diag on integer rows, bit for bit against int64 arithmetic -- a missed or double-counted
    row, a block added to the wrong cell or a stale slot changes an integer;
  * the same on the rows the row kernels wrote, against fp64, within the rounding bound gamma(m_j) mag_j of the operations the
    result went through;
  * the factor form of the rows against the fp64 product of the dense rows of the same sites.

The operator's workspace is scratch without an initial value (nksr_fused_op_t.workspace): every case fills it with NaN bit
patterns first, so a partial block that is read but never written shows (the `clumps` layout found one that way: a workgroup
without rows -- a unit of 700 rows covers its window -- still owns a block of every coarse cell around it, which the per-cell sum
adds; k_fz_cells now writes those blocks as zeros)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_op_ref as fr
import parity_util as pu

pytestmark = pytest.mark.gpu

ALL_LAYOUTS = sorted(fr.LAYOUTS)
_fields = {}


def _dev():
    return torch.device('cuda:0')


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _field(name, approx):
    """KernelField over the layout's hierarchy (built through SparseFeatureHierarchy.build_point_neighborhood) + its site sets"""
    from nksr_amd.fields import KernelField
    from nksr_amd.fields.kernel_field import Segments
    L = fr.layout(name)
    lay = L['layout']
    if name not in _fields:
        oh, svh, feats, _, net = pu.field_inputs(lay.cloud, _dev(), depth=lay.depth, seed=3)
        for d in range(lay.depth):
            assert np.array_equal(svh.level(d).ijk.cpu().numpy(), oh.levels[d].ijk)
        nrm = lay.normal_sites(L['oh'])
        nval = None if nrm is None else np.random.RandomState(5).randn(len(nrm), 3).astype(np.float32)
        seg = None
        if lay.segments:
            k_top, s = svh.level(lay.depth - 1).keys, 3 * (lay.depth - 1)
            h = k_top.numel() // 2
            seg = Segments(svh, torch.stack([k_top[0], k_top[h]]) << s, torch.stack([k_top[h], k_top[-1] + 1]) << s)
        _fields[name] = (svh, feats, net, nrm, nval, seg)
    svh, feats, net, nrm, nval, seg = _fields[name]
    fld = KernelField(svh, net.interpolators, [torch.from_numpy(f) for f in feats], approx_kernel_grad=approx)
    return L, fld, nrm, nval, seg


def _operator(name, approx=False, row_format='dense'):
    L, fld, nrm, nval, seg = _field(name, approx)
    lay = L['layout']
    fld.solver_config['row_format'] = row_format
    wp = 1e4 / max(1, 0 if lay.pos is None else len(lay.pos))
    wn = 1e2 / max(1, 0 if nrm is None else len(nrm))
    pval = None if lay.pos is None else np.random.RandomState(6).randn(len(lay.pos)).astype(np.float32)      # (targets on the position rows too)
    op = fld.fused_operator(_t(lay.pos), _t(nrm), _t(nval), wp, wn, pos_value=_t(pval), segments=seg)
    assert op['row_format'] == row_format
    return L, fld, op


def _workspace(op):
    ws = [b for b in op['keep'] if torch.is_tensor(b) and b.dtype == torch.uint8]
    assert len(ws) == 1
    return ws[0]


def _poison(op):
    _workspace(op).fill_(0xFF)          # fp32 NaN in every word


def _tables_of(op):
    nbr32, nbrT, item_begin, offsets, multi = op['keep'][:5]
    return {'span': op['span'], 'item_begin': item_begin, 'offsets': offsets, 'multi': multi, 'nbr32': nbr32, 'nbrT': nbrT}


def _check_tables(tag, fld, op, rc_ref, T):
    from nksr_amd import _lib
    from nksr_amd._lib import call, ptr, stream
    M, depth, R = fld.svh.num_unknowns, fld.svh.depth, op['rows_total']
    assert R == rc_ref.shape[1], '%s: %d rows, the reference list has %d' % (tag, R, rc_ref.shape[1])
    fr.compare_exact(tag + ':row_cells', op['row_cells'].cpu().numpy().reshape(-1), rc_ref.reshape(-1))
    assert int(_lib.lib.nksr_fused_item_entries(R)) == T['item_begin'].size
    got = _tables_of(op)
    for k in ('span', 'item_begin', 'offsets', 'multi', 'nbr32', 'nbrT'):
        fr.compare_exact('%s:%s' % (tag, k), got[k].cpu().numpy().reshape(-1), T[k].reshape(-1))
    assert (op['nblocks'], op['n_multi'], op['op'].n_big, op['op'].n_multi, op['op'].nblocks) == (T['nblocks'], T['n_multi'], T['n_big'], T['n_multi'], T['nblocks'])
    # counts, straight from the library
    span = torch.full((3, M), -7, dtype=torch.int32, device=_dev())
    counts = torch.full((M + 1,), -7, dtype=torch.int32, device=_dev())
    ib = torch.full((T['item_begin'].size,), -7, dtype=torch.int32, device=_dev())
    call('nksr_fused_block_counts', depth, M, R, ptr(op['row_cells']), ptr(span), ptr(ib), ptr(counts), stream())
    fr.compare_exact(tag + ':counts', counts.cpu().numpy(), T['counts'])
    fr.compare_exact(tag + ':span (direct)', span.cpu().numpy().reshape(-1), T['span'].reshape(-1))
    fr.compare_exact(tag + ':item_begin (direct)', ib.cpu().numpy(), T['item_begin'])
    # the two neighbour tables name each other
    nT, n32 = got['nbrT'].cpu().numpy(), got['nbr32'].cpu().numpy()
    s, j = np.nonzero(nT >= 0)
    assert np.array_equal(n32[nT[s, j], 26 - s], j), tag + ': nbrT[s][j] == c does not imply nbr32[c][26 - s] == j'


@pytest.mark.parametrize('name', ALL_LAYOUTS)
def test_tables_equal_their_restatement_word_for_word(name):
    L, fld, op = _operator(name)
    _check_tables('fused_op[%s]' % name, fld, op, L['row_cells'], L['tables'])


@pytest.mark.parametrize('name', ALL_LAYOUTS)
def test_operator_on_integer_rows_is_exact(name):
    """Rows from {-1, 0, 1}, small integer targets and x: every partial sum is an integer below 2^24 (asserted on the CPU for each
    of these cases), so b, diag, y and the count of non-zero slots must equal the int64 reference bit for bit -- whatever the order
    of the additions.  Two applications with different x on one operator (stale per-cell sums or partial blocks), one after the
    set-up sweep (they share cell_sums and the workspace), reg 1 and 0.5."""
    L, fld, op = _operator(name)
    tag = 'fused_op[%s]:int' % name
    rc, nb, M = L['row_cells'], L['nbr'], L['M']
    fr.compare_exact(tag + ':row_cells', op['row_cells'].cpu().numpy().reshape(-1), rc.reshape(-1))
    rows, t, xs = fr.integer_case(rc, nb, seed=7)
    fld.dense_rows(op).copy_(_t(rows.astype(np.float32)))
    op['targets_all'].copy_(_t(t.astype(np.float32)))
    Rm = fr.rows_matrix(rows, rc, nb, M)
    _poison(op)

    def apply(x, reg):
        ref = fr.operator_ref(rows, rc, nb, t, x, reg, Rm=Rm)
        y = fld.fused_apply(op, _t(x.astype(np.float32)), reg).cpu().numpy()
        fr.compare_exact('%s:y(reg=%g)' % (tag, reg), y * np.float32(ref['scale']), ref['y'])
        return ref

    def setup(reg):
        ref = fr.operator_ref(rows, rc, nb, t, xs[0], reg, Rm=Rm)
        b, diag = fld.fused_rhs_diag(op, reg)
        fr.compare_exact('%s:b' % tag, b.cpu().numpy(), ref['b'])
        fr.compare_exact('%s:diag(reg=%g)' % (tag, reg), diag.cpu().numpy() * np.float32(ref['scale']), ref['diag'])
        fr.compare_exact('%s:nnz' % tag, op['nnz_counter'].cpu().numpy(), np.array([ref['nnz']]))

    apply(xs[0], 1.0)
    apply(xs[1], 0.5)
    setup(1.0)
    apply(xs[2], 1.0)
    _poison(op)
    setup(0.5)
    apply(xs[0], 0.5)
    pu.report(tag, rows=int(rc.shape[1]), M=M, nblocks=op['nblocks'], exact=True)


def _within(tag, got, ref, bound, loose=None):
    """max over the unknowns of |got - ref| / bound (a bound of 0 admits no error) through pu.check against 1; where ``loose`` is
    given, also the largest ratio to that other bound, reported only."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all(), '%s: %d non-finite entries' % (tag, int((~np.isfinite(err)).sum()))
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    if loose is not None:
        # next to the 3e-6 mag_j bound of tests/test_gpu_full_size.py -- reported, not asserted: over the unknowns whose own bound is
        # the tighter one (none, as long as 27 depth + 35 additions make gamma(m_j) >= 3.7e-6), and over all of them
        sel, ref3 = loose[0], np.maximum(loose[1], 1e-300)
        pu.report(tag + ':vs_3e-6_mag', unknowns_with_gamma_below=int(sel.sum()), their_ratio=float((err[sel] / ref3[sel]).max()) if sel.any() else 0.0,
                  ratio_all=float((err / ref3).max()))
    pu.check(tag + ':measured/bound', ratio.max(), 1.0)


def _fp64_case(L, fld, op_dense, seed=11):
    """fp64 reference from the dense rows and targets as the kernels wrote them"""
    rc, nb, M = L['row_cells'], L['nbr'], L['M']
    rows = fld.dense_rows(op_dense).cpu().numpy().astype(np.float64)
    t = op_dense['targets_all'].cpu().numpy().astype(np.float64)
    x = np.random.RandomState(seed).randn(M).astype(np.float32)
    ref = fr.operator_ref(rows, rc, nb, t, x, 1.0)
    assert ref['scale'] == 1 and ref['y'].dtype == np.float64
    return x, ref


def _check_fp(tag, fld, op, x, ref, g, extra=0.0):
    _poison(op)
    y = fld.fused_apply(op, _t(x), 1.0).cpu().numpy()
    b, diag = fld.fused_rhs_diag(op, 1.0)
    y2 = fld.fused_apply(op, _t(x), 1.0).cpu().numpy()
    assert np.array_equal(y.view(np.int32), y2.view(np.int32)), tag + ': the product changed after the set-up sweep'
    tight = g < 3e-6
    _within(tag + ':y', y, ref['y'], (g + extra) * ref['mag'], (tight, 3e-6 * ref['mag']) if extra == 0.0 else None)
    _within(tag + ':b', b.cpu().numpy(), ref['b'], (g + extra) * ref['mag_b'], (tight, 3e-6 * ref['mag_b']) if extra == 0.0 else None)
    _within(tag + ':diag', diag.cpu().numpy(), ref['diag'], (g + extra) * ref['diag'], (tight, 3e-6 * ref['diag']) if extra == 0.0 else None)


@pytest.mark.parametrize('approx', [False, True])
@pytest.mark.parametrize('name', ALL_LAYOUTS)
def test_operator_on_the_kernel_rows_within_its_rounding_bound(name, approx):
    """|y - y_ref|_j <= gamma(m_j) mag_j with gamma(m) = m u / (1 - m u), u = 2^-24 and m_j the additions a product of y_j goes through
    (fused_op_ref.rounding_steps); b and diag the same way."""
    L, fld, op = _operator(name, approx)
    fr.compare_exact('row_cells', op['row_cells'].cpu().numpy().reshape(-1), L['row_cells'].reshape(-1))
    x, ref = _fp64_case(L, fld, op)
    g = fr.gamma(fr.rounding_steps(L['tables'], L['nbr'], L['layout'].depth))
    _check_fp('fused_op[%s,approx=%d]' % (name, approx), fld, op, x, ref, g)


@pytest.mark.parametrize('name', fr.FACTOR_LAYOUTS)
def test_factor_form_matches_the_dense_rows_product(name):
    """NKSR_ROW_FORMAT=factors: the sweep rebuilds the 27 slots from 16-byte records.  y, b and diag against the fp64 product of the
    DENSE rows of the same sites (the product does not depend on the row list: a normal site's header row is zero), bound
    (gamma(m_j) + 1e-5) mag_j -- 1e-5 is what test_fused_operator_matches_the_assembled_matrix[...-factors] allows the rebuilt
    slots; the factor list's own tables against their restatement; nksr_fused_expand_rows from level 0 and from level 2."""
    from nksr_amd._lib import call, stream
    L, fld, opd = _operator(name)
    x, ref = _fp64_case(L, fld, opd)
    del opd
    lay = L['layout']
    _, fld, op = _operator(name, row_format='factors')
    tag = 'fused_op[%s,factors]' % name
    sites, rps = lay.site_sets(L['oh'], rows_per_normal=4)
    rc4, sets4 = fr.row_cells_ref(L['oh'].levels, sites, rps, segment_key_lo=lay.segment_key_lo(L['oh']), with_sets=True)
    T4 = fr.tables_ref(rc4, L['M'], lay.depth, L['nbr'])
    _check_tables(tag, fld, op, rc4, T4)
    if name == 'clumps':
        assert fr.layout_stats(rc4, T=T4)['max_wg_rows'] > fr.RCAP
    g = fr.gamma(fr.rounding_steps(T4, L['nbr'], lay.depth))
    _check_fp(tag, fld, op, x, ref, g, extra=1e-5)
    # the rebuilt rows written out dense: from level 0 and from level 2 the shared levels hold the same bits; header and pad rows are 0
    R = op['rows_total']
    out = {}
    for c0 in (0, 2):
        dense = fld._arm_dense(op, c0)
        dense.fill_(float('nan'))
        call('nksr_fused_expand_rows', C.byref(op['op']), stream())
        op['op'].dense_out = None
        out[c0] = dense.cpu().numpy()
        assert np.isfinite(out[c0]).all(), '%s: expand_rows(dense_from=%d) left rows unwritten' % (tag, c0)
    assert np.array_equal(out[0][2:].view(np.int32), out[2].view(np.int32))
    kind = op['fac_pos'][:R * 4].view(R, 4)[:, 3].contiguous().view(torch.int32).cpu().numpy()
    header = kind == 1
    is_normal = sets4 == (rps.index(4) if 4 in rps else -2)
    assert np.array_equal(header, is_normal & (np.cumsum(is_normal) % 4 == 1)), tag + ': header rows are not every fourth row of the normal sites'
    nocell = (rc4 < 0).all(0)
    assert not out[0][:, header | (sets4 < 0)].any(), tag + ': header or pad rows are not zero'
    assert not out[0][(rc4 < 0)].any(), tag + ': a row without a cell at a level holds values there'
    pu.report(tag + ':expand_rows', rows=R, header_rows=int(header.sum()), pad_rows=int((sets4 < 0).sum()), rows_without_cell=int(nocell.sum()))
