"""The kernel-field kernels alone (csrc/kfield.hip: k_voxel_psi, k_kernel_rows, k_kernel_factors; csrc/evalf.hip: k_evaluate_f and both
k_evaluate_f_grad) against the fp64 definition of tests/kernel_field_ref.py, within its derived bound gamma(m) mag (measured / bound <=
1, reported through parity_util.check).  Every output buffer is NaN-filled and longer than the kernel may write: what lies past the
last row must still be NaN, nothing within may be."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_field_ref as R
import parity_util as pu

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(R.CASES)
K4 = [n for n in NAMES if R.CASES[n][1] == 4]
_fields = {}


def _dev():
    return torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def call(name, *args):
    from nksr_amd._lib import call as c
    c(name, *args)


def ptr(x):
    from nksr_amd._lib import ptr as p
    return p(x)


def stream():
    from nksr_amd._lib import stream as s
    return s()


def setup(name):
    """(case, KernelField with the case's alpha, queries on the device)"""
    if name not in _fields:
        from nksr_amd.fields import KernelField
        c = R.case(name, _dev())
        fld = KernelField(c['svh'], c['net'].interpolators, [torch.from_numpy(f) for f in c['feats']])
        fld.alpha = t(c['alpha'])
        _fields[name] = (c, fld, t(c['q']))
    return _fields[name]


def nan_buf(rows, *tail, extra=3):
    """A NaN-filled buffer of rows + extra rows and its first ``rows`` rows (same start: the 16-byte alignment is the buffer's)."""
    buf = torch.full((rows + extra,) + tail, float('nan'), dtype=torch.float32, device=_dev())
    return buf, buf[:rows]


def host(buf, rows):
    """The first ``rows`` rows on the host, after asserting that they hold no NaN and that everything behind them still is NaN."""
    a = buf.cpu().numpy()
    assert np.isnan(a[rows:]).all(), 'written past the last row'
    assert not np.isnan(a[:rows]).any(), 'NaN (or unwritten) output'
    return a[:rows]


def check(name, got, ref, mag, g, scale=1.0, where=None):
    pu.check(name, R.ratio(got, ref, mag, g, scale, where), 1.0)


# ---- nksr_voxel_psi ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,H', [(4, 16), (16, 32), (4, 32), (16, 16)])
def test_voxel_psi(K, H):
    from nksr_amd.nn.network import Interpolator
    it = Interpolator(K, H, 2, init_scale=R.INIT_SCALE, generator=torch.Generator().manual_seed(K * 100 + H))
    rs = np.random.RandomState(K + H)
    b = [rs.randn(H) * 0.2, rs.randn(H) * 0.2, rs.randn(K) * 0.05]
    W = [it.W1.detach().numpy(), it.W2.detach().numpy(), it.W3.detach().numpy()]
    feat = rs.randn(257, K).astype(F32)
    feat[:, 0] += 1
    lv = R.RefLevel(np.zeros((257, 3)), feat, W[0], b[0].astype(F32), W[1], b[1].astype(F32), W[2], b[2].astype(F32), np.zeros(257))
    psi, mpsi = R.voxel_psi(lv)
    mlp = t(np.concatenate([a.reshape(-1) for a in (W[0], b[0], W[1], b[1], W[2], b[2])]).astype(F32))
    for n in (1, 255, 256, 257):
        buf, out = nan_buf(n, K)
        call('nksr_voxel_psi', ptr(t(feat[:n])), n, K, H, ptr(mlp), ptr(out), stream())
        check('kfield:psi:K%d_H%d:n%d' % (K, H, n), host(buf, n), psi[:n], mpsi[:n], R.gamma(R.psi_chain(K, H)))


@pytest.mark.parametrize('name', NAMES)
def test_the_fields_psi(name):
    c, fld, q = setup(name)
    for d in range(c['depth']):
        check('kfield:%s:psi%d' % (name, d), fld._psi[d].cpu().numpy(), c['ref'].lv[d]['psi'], c['ref'].lv[d]['mpsi'], R.gamma(R.psi_chain(c['K'], c['H'])))


# ---- nksr_kernel_rows -------------------------------------------------------------------------------------------------------------------
def rows_direct(fld, q, n, approx, scale=1.0, site_scale=None, val=None, dval=None):
    call('nksr_kernel_rows', C.byref(fld._hier), ptr(q), n, int(approx), float(scale), ptr(site_scale), 0, None, None, ptr(val), ptr(dval), stream())


def check_rows(tag, ref, n, val=None, dval=None, exact=True, scale=1.0):
    """site-major rows [n, L, 27] / [n, 3, L, 27] (host) against the reference; ``scale``: a number or one per site"""
    rows = ref.rows(exact)
    g = ref.g
    s = np.asarray(scale, np.float64).reshape(-1)
    if val is not None:
        sv = s.reshape(-1, 1, 1)
        assert (val[rows['cols'] < 0] == 0).all(), 'an absent slot or a row of an inactive cell is not 0'
        check(tag + ':val', val, rows['val'] * sv, rows['mval'] * np.abs(sv), g)
    if dval is not None:
        sv = s.reshape(-1, 1, 1, 1)
        gone = np.broadcast_to((rows['cols'] < 0)[:, None], dval.shape)
        assert (dval[gone] == 0).all(), 'an absent slot or a row of an inactive cell is not 0'
        check(tag + ':dval_' + ('exact' if exact else 'approx'), dval, rows['dval'] * sv, rows['mdval'] * np.abs(sv), g,
              where=ref.trusted(True) if exact else None)


def level_major(out, ri, ncomp):
    """[L, stride, 27] with site i at rows ri[i] .. ri[i] + ncomp - 1 -> site-major [n, (ncomp,) L, 27]"""
    if ncomp == 1:
        return out[:, ri].transpose(1, 0, 2)
    return np.stack([out[:, ri + a] for a in range(ncomp)], 0).transpose(2, 0, 1, 3)


@pytest.mark.parametrize('name', NAMES)
def test_kernel_rows(name):
    c, fld, q = setup(name)
    ref, n, L = c['ref'], len(c['q']), c['depth']
    rs = np.random.RandomState(11)
    # val and dval (exact) in one launch, site-major
    vb, v = nan_buf(n, L, 27)
    db, dv = nan_buf(n, 3, L, 27)
    rows_direct(fld, q, n, False, val=v, dval=dv)
    val, dval = host(vb, n), host(db, n)
    check_rows('kfield:%s:rows' % name, ref, n, val, dval, exact=True)
    # through KernelField.kernel_rows: the same numbers
    fld.approx_kernel_grad = False
    wv, wd = fld.kernel_rows(q, grad=True)
    assert torch.equal(wv, v) and torch.equal(wd, dv)
    # dval approx, values=False, row_scale != 1
    db, dv = nan_buf(n, 3, L, 27)
    rows_direct(fld, q, n, True, scale=-1.75, dval=dv)
    check_rows('kfield:%s:rows_scaled' % name, ref, n, None, host(db, n), exact=False, scale=-1.75)
    fld.approx_kernel_grad = True
    wv, wd = fld.kernel_rows(q, grad=True, scale=-1.75, values=False)
    fld.approx_kernel_grad = False
    assert wv is None and torch.equal(wd, dv)
    # a per-site scale (row_scale is then ignored)
    ss = (0.5 + 1.5 * rs.rand(n)).astype(F32)
    vb, v = nan_buf(n, L, 27)
    rows_direct(fld, q, n, False, scale=123.0, site_scale=t(ss), val=v)
    check_rows('kfield:%s:rows_site_scale' % name, ref, n, host(vb, n), scale=ss)
    # level-major with a permuted row_index and row_cells: value rows, then exact gradient rows
    cell = ref.rows(True)['cell']
    for grad, ncomp in ((False, 1), (True, 3)):
        stride = ncomp * (n + 4)
        ri = (rs.permutation(n + 4)[:n] * ncomp).astype(np.int32)
        out = torch.full((L, stride, 27), float('nan'), dtype=torch.float32, device=_dev())
        rc = torch.full((L, stride), -7, dtype=torch.int32, device=_dev())
        fld.kernel_rows_level_major(q, grad, 1.0, out, stride, row_index=t(ri), row_cells=rc, site_scale=t(ss))
        o, rcn = out.cpu().numpy(), rc.cpu().numpy()
        written = np.zeros(stride, bool)
        for a in range(ncomp):
            written[ri + a] = True
            assert np.array_equal(rcn[:, ri + a].T, cell), 'row_cells'
        assert np.isnan(o[:, ~written]).all() and (rcn[:, ~written] == -7).all(), 'rows of no site were written'
        assert not np.isnan(o[:, written]).any()
        got = level_major(o, ri, ncomp)
        if grad:
            check_rows('kfield:%s:rows_level_major' % name, ref, n, None, got, exact=True, scale=ss)
        else:
            check_rows('kfield:%s:rows_level_major' % name, ref, n, got, scale=ss)


# ---- nksr_kernel_factors (kernel_dim 4) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', K4)
def test_kernel_factors(name):
    c, fld, q = setup(name)
    ref, n, L = c['ref'], len(c['q']), c['depth']
    rs = np.random.RandomState(12)
    g = ref.g
    active = np.stack([Rl['active'] for Rl in ref.lv], 1)                                         # [n, L]
    phi = np.stack([Rl['phi'] for Rl in ref.lv], 1) * active[..., None]                           # [n, L, 4]
    mphi = np.stack([Rl['mphi'] for Rl in ref.lv], 1) * active[..., None]
    J = np.stack([Rl['J'] for Rl in ref.lv], 1) * active[..., None, None]                         # [n, L, 4, 3]
    mJ = np.stack([Rl['mJ'] for Rl in ref.lv], 1) * active[..., None, None]
    cell = ref.rows(True)['cell']
    scale = 1.5
    for grad, approx in ((False, False), (True, False), (True, True)):
        nr = 4 if grad else 1
        stride = nr * (n + 4)
        ri = (rs.permutation(n + 4)[:n] * nr).astype(np.int32)
        vec = torch.full((L, stride, 4), float('nan'), dtype=torch.float32, device=_dev())
        pos = torch.full((stride, 4), float('nan'), dtype=torch.float32, device=_dev())
        rc = torch.full((L, stride), -7, dtype=torch.int32, device=_dev())
        fld.approx_kernel_grad = approx
        fld.kernel_factors_level_major(q, grad, scale, vec, pos, stride, row_index=t(ri), row_cells=rc)
        fld.approx_kernel_grad = False
        v, p, rcn = vec.cpu().numpy(), pos.cpu().numpy(), rc.cpu().numpy()
        written = np.zeros(stride, bool)
        tag = 'kfield:%s:factors_%s' % (name, ('approx' if approx else 'exact') if grad else 'value')
        for k in range(nr):
            written[ri + k] = True
            assert np.array_equal(rcn[:, ri + k].T, cell), 'row_cells'
            assert np.array_equal(p[ri + k, :3].view(np.int32), ref.p32.view(np.int32)), 'pos is not the fp32 product p bit for bit'
            # kind bits (include/nksr_hip.h): 0 position row, 1 header row of a normal site, 2 + a gradient row of axis a
            assert (p[ri + k, 3].view(np.int32) == (1 + k if grad else 0)).all(), 'kind bits'
        assert np.isnan(v[:, ~written]).all() and np.isnan(p[~written]).all() and (rcn[:, ~written] == -7).all()
        assert not np.isnan(v[:, written]).any()
        check(tag + ':phi', v[:, ri].transpose(1, 0, 2), phi, mphi, g, scale)
        for a in range(3 if grad else 0):
            got = v[:, ri + 1 + a].transpose(1, 0, 2)
            if approx:
                assert (got == 0).all(), 'J rows of the approximate gradient are not 0'
            else:
                check(tag + ':J%d' % a, got, J[..., a], mJ[..., a], g, scale, where=ref.trusted(True))


# ---- nksr_evaluate_f: k_evaluate_f, k_evaluate_f_grad<JAC>, k_evaluate_f_grad<!JAC> ------------------------------------------------------
KERNELS = (('value', False, False), ('grad_approx', True, True), ('grad_exact', True, False))


def evaluate_direct(fld, alpha, q, n, grad, approx, active_only):
    """alpha None: the production path (psi pre-multiplied, KernelField._alpha_hier); else a tensor of its own"""
    hier = fld._alpha_hier(fld.alpha) if alpha is None else fld._hier
    fb, f = nan_buf(n)
    gb, g = nan_buf(n, 3) if grad else (None, None)
    call('nksr_evaluate_f', C.byref(hier), ptr(alpha), ptr(q), n, int(approx), int(active_only), ptr(f), ptr(g), stream())
    return host(fb, n), host(gb, n) if grad else None


def check_evaluate(tag, ref, f, g, exact, active_only, alpha=None):
    fv, fm = ref.value(alpha, active_only)
    check(tag + ':f', f, fv, fm, ref.g)
    far = np.abs(ref.p32).max(1) >= 400.0
    assert (f[far] == 0).all()
    if g is not None:
        gv, gm = ref.gradient(exact, alpha, active_only)
        check(tag + ':grad', g, gv, gm, ref.g, where=ref.trusted(active_only) if exact else None)
        assert (g[far] == 0).all()


@pytest.mark.parametrize('name', NAMES)
def test_evaluate_f(name):
    c, fld, q = setup(name)
    ref, n = c['ref'], len(c['q'])
    assert (np.abs(ref.p32).max(1) >= 400.0).sum() == 3
    other = t(c['alpha'][::-1].copy())                       # a tensor that is not fld.alpha, with other numbers
    for active_only in (0, 1):
        for mode, alpha in (('null', None), ('given', other)):
            values = {}
            for kname, grad, approx in KERNELS:
                f, g = evaluate_direct(fld, alpha, q, n, grad, approx, active_only)
                values[kname] = f
                check_evaluate('kfield:%s:evaluate_%s:alpha_%s:active_only%d' % (name, kname, mode, active_only), ref, f, g, not approx,
                               bool(active_only), None if alpha is None else c['alpha'][::-1])
            pu.report('kfield:%s:evaluate:alpha_%s:active_only%d' % (name, mode, active_only),
                      value_kernel_bitwise_equals_grad_kernel=bool(np.array_equal(values['value'], values['grad_exact'])),
                      grad_kernels_bitwise_equal=bool(np.array_equal(values['grad_approx'], values['grad_exact'])))


# ---- launch shapes: the block edge, one site, and the max_points slicing of _evaluate_raw ------------------------------------------------
@pytest.mark.parametrize('name', ['diagonal_negative', 'two_clusters'])
def test_block_edges_and_slicing(name):
    c, fld, q = setup(name)
    L = c['depth']
    for n in (1, 127, 128, 129):
        ref = c['ref'].take(slice(0, n))
        qn = q[:n].contiguous()
        tag = 'kfield:%s:n%d' % (name, n)
        vb, v = nan_buf(n, L, 27)
        db, dv = nan_buf(n, 3, L, 27)
        rows_direct(fld, qn, n, False, val=v, dval=dv)
        check_rows(tag + ':rows', ref, n, host(vb, n), host(db, n), exact=True)
        for kname, grad, approx in KERNELS:
            f, g = evaluate_direct(fld, None, qn, n, grad, approx, 0)
            check_evaluate(tag + ':evaluate_' + kname, ref, f, g, not approx, False)
        if c['K'] == 4:
            vec = torch.full((L, n + 3, 4), float('nan'), dtype=torch.float32, device=_dev())
            pos = torch.full((n + 3, 4), float('nan'), dtype=torch.float32, device=_dev())
            fld.kernel_factors_level_major(qn, False, 1.0, vec, pos, n + 3)
            v = vec.cpu().numpy()
            assert np.isnan(v[:, n:]).all() and np.isnan(pos.cpu().numpy()[n:]).all()
            active = np.stack([Rl['active'] for Rl in ref.lv], 1)[..., None]
            check(tag + ':factors_phi', v[:, :n].transpose(1, 0, 2), np.stack([Rl['phi'] for Rl in ref.lv], 1) * active,
                  np.stack([Rl['mphi'] for Rl in ref.lv], 1) * active, ref.g)
    # the wrappers: evaluate_f (production path, alpha == NULL) and _evaluate_raw in slices of 100
    n = 257
    ref = c['ref'].take(slice(0, n))
    qn = q[:n].contiguous()
    other = c['alpha'][::-1].copy()
    for approx in (False, True):
        fld.approx_kernel_grad = approx
        tag = 'kfield:%s:n257_%s' % (name, 'approx' if approx else 'exact')
        res = fld.evaluate_f(qn, grad=False)
        assert res.gradient is None
        check_evaluate(tag + ':evaluate_f_value', ref, res.value.cpu().numpy(), None, not approx, False)
        res = fld.evaluate_f(qn, grad=True)
        check_evaluate(tag + ':evaluate_f_grad', ref, res.value.cpu().numpy(), res.gradient.cpu().numpy(), not approx, False)
        for grad in (False, True):
            for alpha_t, alpha in ((fld.alpha, None), (t(other), other)):
                for active_only in (False, True):
                    res = fld._evaluate_raw(alpha_t, qn, grad, max_points=100, active_only=active_only)
                    whole = fld._evaluate_raw(alpha_t, qn, grad, active_only=active_only)
                    assert torch.equal(res.value, whole.value) and (not grad or torch.equal(res.gradient, whole.gradient))
                    check_evaluate(tag + ':sliced_grad%d_%s_active_only%d' % (grad, 'null' if alpha is None else 'given', active_only), ref,
                                   res.value.cpu().numpy(), res.gradient.cpu().numpy() if grad else None, not approx, active_only, alpha)
    fld.approx_kernel_grad = False
