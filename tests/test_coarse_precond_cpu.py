"""The references of tests/test_gpu_coarse_precond.py checked against each other, without a GPU: what the GPU tests compare the
kernels with is itself verified here, and the fp32 rounding floor that their bounds are multiples of is printed per case."""
import numpy as np
import pytest

import coarse_precond_ref as R

FORMATS = [(0, 0.0), (1, 0.0), (1, R.DROP)]
IDS = ['plain', 'packed-drop0', 'packed-drop']


def test_block_set_covers_the_shapes_the_kernels_turn_on():
    """n around 16 / 64 / 256 rows, every trip count of a row, one and three interleaved segments, a one-row segment, a dead tail in
    the last wavefront, an empty row beside a long one in one 4-row group of the packed step -- before and after the drop."""
    ns = sorted(R.block(k)['n'] for k in R.BLOCKS)
    assert ns[:7] == [1, 15, 16, 17, 64, 65, 257] and 1400 <= ns[7] <= 1600 and ns[7] % 16 != 0
    assert {R.block(k)['nseg'] for k in R.BLOCKS} == {1, 3}
    lens = set()
    for k in R.BLOCKS:
        b = R.block(k)
        lens |= set((np.diff(b['rowptr']) - 1).tolist())
        assert (b['cols'][b['rowptr'][1:] - 1] == np.arange(b['n'])).all()                  # the diagonal closes every row
        assert np.array_equal(b['vals'][b['rowptr'][1:] - 1], b['diag'])
        assert np.array_equal(b['dense'], b['dense'].T)                                      # bitwise symmetric fp32 values
        if b['nseg'] == 3:
            counts = np.bincount(b['row_seg'])
            assert counts.min() == 1                                                         # one segment is a single row
            assert (np.diff(b['row_seg']) < 0).any()                                         # interleaved: old_of_new is a real permutation
            lam = R.prepared(k, 0)['lam']
            assert len(set(lam.tolist())) == 3, lam                                          # every segment its own interval
    assert lens >= {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257} and max(lens) > 300, sorted(lens)
    for drop in (0.0, R.DROP):
        pk = R.prepared('n1501x3', 1, drop)['pk']
        kept = pk['lens']
        groups = kept[:len(kept) // 4 * 4].reshape(-1, 4)
        assert ((groups.min(1) == 0) & (groups.max(1) > 64)).any(), 'no empty row beside a long one'
        assert (kept == 0).mean() >= (0.05 if drop else 0.0) and kept.max() > 64
        # the matrix is ill-conditioned for the interval: lmax / lmin well above the ratio
        w = R.prepared('n1501x3', 1, drop)['eigs'][0][1]
        assert w[0] > 0 and w[-1] / w[0] > 5 * R.RATIO
    assert (R.prepared('n1501x3', 1, R.DROP)['pk']['lens'] == 0).mean() >= 0.09            # "a tenth of the rows keep no entry"


@pytest.mark.parametrize('fmt,drop', FORMATS, ids=IDS)
@pytest.mark.parametrize('name', list(R.BLOCKS))
def test_recurrence_equals_closed_form(name, fmt, drop):
    """The fp64 recurrence with the fp32-rounded table against the eigen-decomposition formula: they differ by the rounding of the
    2 k + 1 coefficients only.  Bound 2e-7 of max |z| = 3 x 2^-24, one fp32 rounding in each of the three coefficients a value passes
    through per step at the worst (measured: <= 5.6e-8 over all cases).  The fp32 recurrence's own error -- the rounding floor the GPU
    tests scale their bounds from -- is printed (measured: 6.0e-8 .. 5.4e-7)."""
    prep = R.prepared(name, fmt, drop)
    r = R.rhs(prep['blk']['n'])
    for steps in R.STEPS:
        zref = R.reference(prep, r, steps)
        e64 = R.rel_err(R.reference(prep, r, steps, dtype=np.float64), zref, prep['blk']['row_seg'])
        _, floor = R.rounding_floor(prep, r, steps)
        print('[coarse_precond_ref] %s fmt=%d drop=%g steps=%d: fp64 recurrence vs closed form %.2e, fp32 rounding floor %.2e' % (name, fmt, drop, steps, e64, floor))
        assert e64 <= 2e-7, (steps, e64)
        assert floor <= 2e-6, (steps, floor)             # a floor this large would make 8 x floor admit real mistakes


def test_coefficient_table():
    """cheb_coeffs against an independent statement: the residual polynomial of the recurrence with these coefficients is
    T_k((theta - l) / delta) / T_k(theta / delta) -- checked on scalars (a 1 x 1 system per l) -- and the degenerate / capped rules."""
    lam = np.array([1.7, 0.0, -1.0, np.inf, np.nan, 2.5], np.float32)
    gersh = np.array([5.0, 5.0, 5.0, 5.0, 5.0, 2.0], np.float32)
    top = R.interval_top(lam, gersh, 1.1)
    assert np.isnan(top[[1, 2, 4]]).all() and top[0] == np.float64(np.float32(1.1)) * np.float64(np.float32(1.7)) and top[5] == 2.0
    assert top[3] == 5.0                      # an infinite estimate is capped like any other: without a cap it is degenerate
    assert np.isnan(R.interval_top(lam, None, 1.1)[1:5]).all()
    assert np.array_equal(R.interval_top(lam, None, 1.1)[[0, 5]], np.float64(np.float32(1.1)) * lam[[0, 5]].astype(np.float64))
    for steps in R.STEPS:
        coef = R.cheb_coeffs(lam, gersh, 1.1, 40.0, steps)
        for c in (1, 2, 4):
            assert coef[c, 0] == 1.0 and not coef[c, 1:].any()
        assert not coef[:, 1 + 2 * steps:].any()
        for c in (0, 3, 5):
            ls = np.linspace(0.01, 1.5, 300) * top[c]
            d = coef[c, 0].astype(np.float64) * np.ones_like(ls)       # A = l, D = 1, r = 1
            res, y = np.ones_like(ls), np.zeros_like(ls)
            for i in range(steps):
                y, res = y + d, res - ls * d
                d = coef[c, 1 + 2 * i].astype(np.float64) * d + coef[c, 2 + 2 * i].astype(np.float64) * res
            p = R.poly(ls, top[c], 40.0, steps)
            assert np.abs(y - p).max() <= 3e-7 * np.abs(p).max()


@pytest.mark.parametrize('fmt,drop', FORMATS, ids=IDS)
def test_polynomial_is_positive_with_the_margin_and_not_with_a_quarter(fmt, drop):
    """p > 0 on the whole spectrum with lambda_scale = 1.1 (the preconditioner is SPD), p < 0 somewhere with 0.25 and an even
    number of steps: what the Jacobi fallback of the solve, and the GPU test of it, rely on."""
    prep = R.prepared('n1501x3', fmt, drop)
    for steps in R.STEPS:
        for (rows, w, U), lmax in zip(prep['eigs'], R.interval_top(prep['lam'], None, 1.1)):
            assert (R.poly(w, lmax, R.RATIO, steps) > 0).all()
    for (rows, w, U), lmax in zip(prep['eigs'], R.interval_top(prep['lam'], None, 0.25)):
        if len(rows) > 1:
            assert (R.poly(w, lmax, R.RATIO, 8) < 0).any()


@pytest.mark.parametrize('name', list(R.BLOCKS))
def test_packed_matrix_is_symmetric_and_no_decision_sits_on_the_drop_tolerance(name):
    blk = R.block(name)
    for drop in (0.0, R.DROP):
        pk = R.prepared(name, 1, drop)['pk']
        assert np.array_equal(pk['S_h'], pk['S_h'].T)                   # exactly
        assert (np.diag(pk['S_h']) == 1.0).all()
        assert pk['packed_rowptr'][-1] == len(pk['packed']) == pk['lens'].sum()
        assert np.array_equal(np.sort(pk['old_of_new']), np.arange(blk['n'])) and np.array_equal(pk['new_of_old'][pk['old_of_new']], np.arange(blk['n']))
        assert (np.diff(pk['row_seg_new']) >= 0).all()
        # the words decode to S_h
        rows = pk['old_of_new'][np.repeat(np.arange(blk['n']), pk['lens'])]
        cols = pk['old_of_new'][(pk['packed'] & 0xFFFF).astype(np.int64) + pk['seg_base'][pk['row_seg_new'][np.repeat(np.arange(blk['n']), pk['lens'])]]]
        vals = (pk['packed'] >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
        back = np.eye(blk['n'])
        back[rows, cols] = vals
        assert np.array_equal(back, pk['S_h'])
    # every fp32 scaled entry lies more than one half-precision ulp (at the tolerance) away from the tolerance: the kept / dropped
    # pattern does not hang on the last bit of 1 / sqrt or of a product  (measured: 2.3 half ulps on n1501x3, > 1000 elsewhere)
    margin = R.drop_margin(R.prepared(name, 1, R.DROP)['pk']['s32'], R.DROP)
    print('[coarse_precond_ref] %s: nearest entry to the drop tolerance: %.2f half ulps' % (name, margin))
    assert margin > 1.0
    if blk['n'] > 64:
        kept = R.prepared(name, 1, R.DROP)['pk']['lens'].sum()
        assert 0 < kept < R.prepared(name, 1, 0.0)['pk']['lens'].sum()          # the tolerance does drop, and not everything


def test_eigenvalue_bounds_of_the_reference_are_ordered():
    """power estimate <= lambda_max <= Gershgorin.  For the packed block this is a theorem (S_h is symmetric: the estimate is the
    root of a Rayleigh quotient of S_h^2), asserted on every block.  For the plain block the iteration runs on D^-1 A, similar to S but
    not symmetric, and the 2-norm ratio may overshoot: n16 gives 1.0095 x lambda_max, n17x3 1.0003 x (fp64).  That errs on the safe
    side (a larger interval keeps the polynomial positive) but the order is no theorem there, so the GPU test of the order runs on
    R.BOUND_BLOCKS, where the reference itself keeps it -- asserted here (measured: estimate / lambda_max in 0.86 .. 1.0)."""
    for name in list(R.BLOCKS) + ['ranges']:
        for fmt, drop in FORMATS:
            prep = R.prepared(name, fmt, drop)
            blk = prep['blk']
            true = R.lambda_true(prep['S'], blk['row_seg'])
            if fmt == 0:
                est = R.power_plain(blk, 8, row_seg=blk['row_seg'])
                g = R.gersh_ref(blk=blk, row_seg=blk['row_seg'])
            else:
                est, g = R.power_packed(prep['pk'], 8), R.gersh_ref(pk=prep['pk'])
            print('[coarse_precond_ref] %s fmt=%d drop=%g: power / true %s, gershgorin / true %s' % (name, fmt, drop, np.round(est / true, 4), np.round(g / true, 3)))
            assert (true <= g * (1 + 1e-5)).all(), (name, fmt, true, g)
            if fmt == 1 or name in R.BOUND_BLOCKS:
                assert (est <= true * (1 + 1e-5)).all(), (name, fmt, est, true)
            assert (est <= true * 1.02).all()
            if fmt == 0 and name in R.BOUND_BLOCKS:           # the call without segments: one ratio over the whole block
                whole = R.power_plain(blk, 8)
                assert len(whole) == 1 and whole[0] <= true.max() * (1 + 1e-5), (name, whole, true)


def test_ranges_block_is_what_the_segments_struct_describes():
    blk, first, lo, hi = R.ranges_block()
    lo, hi = lo.reshape(4, 3), hi.reshape(4, 3)
    seg_of = np.full(first + blk['n'], -1)
    for c in range(4):
        for k in range(3):
            assert (seg_of[lo[c, k]:hi[c, k]] == -1).all()
            seg_of[lo[c, k]:hi[c, k]] = c
    assert (seg_of >= 0).all() and np.array_equal(seg_of[first:], blk['row_seg'])
    assert (hi[3, 1:] == lo[3, 1:]).all() and hi[3, 0] > lo[3, 0]           # segment 3: no coarse rows
    assert (np.diff(blk['row_seg']) < 0).any()
