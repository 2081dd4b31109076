"""tests/kernel_field_ref.py without a GPU: the fp32 oracle (the stencil form: cells, half bits, slots) meets the derived bound of the
brute-force fp64 definition on every case, so the bound is neither vacuous nor out of reach and the two statements say the same; the
cases hold the queries they are meant to hold; and wrong evaluations -- the oracle with one thing changed -- miss the bound by 10 x."""
import types

import numpy as np
import pytest

import kernel_field_ref as R
from oracle import field, kernel, spec

F32 = np.float32
NAMES = list(R.CASES)


def oracle_ratios(c):
    """measured / bound of every output of the fp32 oracle on a case: {what: ratio}."""
    ref, oh, feats, oi, q, alpha = c['ref'], c['oh'], c['feats'], c['ointerps'], c['q'], c['alpha']
    g = ref.g
    psis = [kernel.voxel_psi(feats[d], oi[d]) for d in range(c['depth'])]
    out = {}
    for d in range(c['depth']):
        out['psi%d' % d] = R.ratio(psis[d], ref.lv[d]['psi'], ref.lv[d]['mpsi'], R.gamma(R.psi_chain(c['K'], c['H'])))
    for exact in (True, False):
        tag = 'exact' if exact else 'approx'
        rows = ref.rows(exact)
        cols, val, dval = kernel.kernel_rows(oh, feats, oi, psis, q, True, not exact)
        assert np.array_equal(cols, rows['cols']), 'columns differ'
        ok = ref.trusted(True) if exact else None
        out['rows_val'] = R.ratio(val, rows['val'], rows['mval'], g)
        out['rows_dval_' + tag] = R.ratio(dval, rows['dval'], rows['mdval'], g, where=ok)
        # the rows' support (active_only) from the rows themselves, the full support from the oracle's evaluate_f
        a = np.where(cols >= 0, alpha[np.maximum(cols, 0)], F32(0)).astype(np.float64)
        fv, fm = ref.value(active_only=True)
        gv, gm = ref.gradient(exact, active_only=True)
        out['f_active_only'] = R.ratio((a * val).sum((1, 2)), fv, fm, g)
        out['grad_active_only_' + tag] = R.ratio((a[:, None] * dval).sum((2, 3)), gv, gm, g, where=ok)
        fo, go = field.evaluate_f(oh, feats, oi, psis, alpha, q, True, not exact)
        fv, fm = ref.value()
        gv, gm = ref.gradient(exact)
        out['f'] = R.ratio(fo, fv, fm, g)
        out['grad_' + tag] = R.ratio(go, gv, gm, g, where=ref.trusted(False) if exact else None)
    return out


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_meets_the_bound_and_the_case_holds_its_queries(name):
    c = R.case(name)
    ratios = oracle_ratios(c)
    worst = max(ratios, key=ratios.get)
    print('[kernel_field_ref] %s: m=%d gamma=%.3e worst measured/bound %.3e (%s)' % (name, c['ref'].m, c['ref'].g, ratios[worst], worst))
    assert ratios[worst] <= 1.0, ratios
    assert min(ratios.values()) >= 0.0 and max(v for k, v in ratios.items() if k.startswith('f')) > 0.0       # (something was compared)
    fallback, on_plane, excluded = R.case_conditions(c)
    print('[kernel_field_ref] %s: queries=%d fallback=%d on_plane=%d excluded=%.3f voxels=%d' % (
        name, len(c['q']), fallback, on_plane, excluded, c['oh'].num_unknowns))
    assert fallback >= R.MIN_FALLBACK and on_plane >= R.MIN_ON_PLANE
    assert excluded <= R.MAX_EXCLUDED
    assert 250 <= len(c['q']) <= 350 and np.isfinite(c['q']).all()
    # far queries: nothing within reach at any level
    far = np.abs(c['q']).max(1) >= 49.0
    assert far.sum() == 3 and (c['ref'].value()[1][far] == 0).all()


def test_the_reference_is_exact_where_the_definition_is_simple():
    """At a voxel centre of a level the trilinear stencil collapses onto that voxel: t = feat_j and phi = psi_j; at the centre the
    spline weight of the voxel itself is 0.75^3 and the gradient of B vanishes there."""
    c = R.case('one_point')
    oh, ref0 = c['oh'], c['ref']
    centres = oh.levels[0].centers()
    ref = R.FieldRef(ref0.levels, centres)
    on = (ref.p32.astype(np.float64) == oh.levels[0].ijk + 0.5).all(1)          # (where the fp32 product lands on the centre exactly)
    assert on.sum() >= 9
    R0 = ref.lv[0]
    j = np.nonzero(on)[0]
    assert np.array_equal(R0['cell'][j], j)
    np.testing.assert_array_equal(R0['t'][j], ref.levels[0].feat[j])
    np.testing.assert_array_equal(R0['phi'][j], R0['psi'][j])
    np.testing.assert_allclose(R0['Kv'][j, j], (R0['psi'][j] ** 2).sum(1) * 0.75 ** 3, rtol=1e-14)
    # the rows are the field: sum over the slots with alpha = f of the active_only support
    rows = ref0.rows(True)
    a = np.where(rows['cols'] >= 0, c['alpha'].astype(np.float64)[np.maximum(rows['cols'], 0)], 0.0)
    np.testing.assert_allclose((a * rows['val']).sum((1, 2)), ref0.value(active_only=True)[0], rtol=0, atol=1e-13)
    np.testing.assert_allclose((a[:, None] * rows['dval']).sum((2, 3)), ref0.gradient(True, active_only=True)[0], rtol=0, atol=1e-11)


def test_the_exact_gradient_is_the_derivative_of_the_value():
    """Central differences of the fp64 value in p, at queries where the field is smooth across the difference: no half-cell plane
    and no ReLU kink between the two ends."""
    c = R.case('two_clusters')
    ref0 = c['ref']
    rs = np.random.RandomState(0)
    q = (c['xyz'][rs.randint(0, len(c['xyz']), 40)] + rs.randn(40, 3) * 0.05).astype(F32)
    ref = R.FieldRef(ref0.levels, q)
    h = 2.0 ** -12                                             # in units of p; exactly representable next to p
    p = ref.p32.astype(np.float64)
    frac = np.abs((p * 2.0) - np.round(p * 2.0))
    smooth = (frac > 4 * h).all(1)
    inv_w0 = float(spec.inv_w0_f32(R.VOXEL))
    grad = ref.gradient(True)[0]
    for a in range(3):
        e = np.zeros(3, F32)
        e[a] = h
        lo, hi = (ref.p32 - e).astype(F32), (ref.p32 + e).astype(F32)
        ok = smooth & (lo.astype(np.float64) == p - e).all(1) & (hi.astype(np.float64) == p + e).all(1)
        rlo, rhi = R.FieldRef(ref0.levels, None, p32=lo), R.FieldRef(ref0.levels, None, p32=hi)
        for d in range(ref.depth):
            ok &= (rlo.lv[d]['masks'] == ref.lv[d]['masks']).all(1) & (rhi.lv[d]['masks'] == ref.lv[d]['masks']).all(1)
        assert ok.sum() >= 15
        num = (rhi.value()[0] - rlo.value()[0]) / (2 * h) * inv_w0
        assert np.abs(num[ok] - grad[ok, a]).max() <= 1e-3 * np.abs(grad[ok]).max(), a


# ---- sensitivity: the oracle with one thing wrong must miss the bound by 10 x ----------------------------------------------------------
def _swap_spline_slots(monkeypatch, c):
    """two B-spline slots (offsets -1 and 0) swapped along the x axis"""
    orig, calls = spec.bspline3, [0]

    def bspline3(u):
        w, dw = orig(u)
        calls[0] += 1
        if calls[0] % 3 == 1:                                # kernel_rows asks for x, y, z in turn
            w, dw = w[..., [1, 0, 2]], dw[..., [1, 0, 2]]
        return w, dw
    monkeypatch.setattr(spec, 'bspline3', bspline3)


def _left_derivative(monkeypatch, c):
    """the left instead of the right derivative of hat at u = 0.5: the half bit of the lower half cell there"""
    oh = c['oh']
    orig = oh.site_cells

    def site_cells(xyz):
        return [(cell, u, np.where(u == F32(0.5), 0, hb).astype(np.int32)) for cell, u, hb in orig(xyz)]
    monkeypatch.setattr(oh, 'site_cells', site_cells)


def _absent_corner_reads_voxel_0(monkeypatch, c):
    """an absent corner of the trilinear stencil read as voxel 0 with its real weight (the 27 slots keep the true tables)"""
    oh = c['oh']
    true_cells = oh.site_cells(c['q'])
    tables = {id(L): (L.nbr, L.lookup) for L in oh.levels}

    def _nbr(L, ijk_cell, cell, s, o, fallback):
        nbr, lookup = tables[id(L)]
        ok = cell >= 0
        j = np.where(ok, nbr[np.where(ok, cell, 0), s], -1)
        return np.where(ok, j, lookup(ijk_cell + o[None])) if fallback and (~ok).any() else j
    monkeypatch.setattr(kernel, '_nbr', _nbr)
    monkeypatch.setattr(oh, 'site_cells', lambda xyz: true_cells)
    for L in oh.levels:
        monkeypatch.setattr(L, 'nbr', np.maximum(L.nbr, 0))
        monkeypatch.setattr(L, 'lookup', lambda ijk, f=L.lookup: np.maximum(f(ijk), 0))


def _drop_the_J_term(monkeypatch, c):
    """the exact gradient without the d(phi)/dx term"""
    orig = kernel.site_features
    monkeypatch.setattr(kernel, 'site_features', lambda hier, feats, interps, xyz, need_jac, fallback=False: orig(hier, feats, interps, xyz, False, fallback))


def _inv_w_of_the_finer_level(monkeypatch, c):
    """the level-d inv_w of level d - 1 (twice as large); the cells still come from the true product"""
    proxy = types.SimpleNamespace(**{k: getattr(spec, k) for k in dir(spec) if not k.startswith('__')})
    proxy.inv_w0_f32 = lambda vs: F32(2.0) * spec.inv_w0_f32(vs)
    monkeypatch.setattr(kernel, 'spec', proxy)


MUTATIONS = [_swap_spline_slots, _left_derivative, _absent_corner_reads_voxel_0, _drop_the_J_term, _inv_w_of_the_finer_level]


@pytest.mark.parametrize('mutate', MUTATIONS, ids=lambda f: f.__name__.strip('_'))
def test_a_wrong_evaluation_misses_the_bound(mutate, monkeypatch):
    worst = {}
    for name in ('one_point', 'diagonal_negative', 'depth1_k16'):
        c = R.case(name)
        with monkeypatch.context() as mp:
            mutate(mp, c)
            try:
                ratios = oracle_ratios(c)
            except AssertionError:                           # (columns differ: the mutation changed the support itself)
                ratios = {'cols': np.inf}
        worst[name] = max(ratios.values())
    print('[kernel_field_ref] mutation %s: measured/bound %s' % (mutate.__name__, {k: '%.2e' % v for k, v in worst.items()}))
    assert max(worst.values()) >= 10.0, worst
