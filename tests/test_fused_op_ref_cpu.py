"""The reference of the matrix-free operator tests (tests/fused_op_ref.py) checked by itself, without a GPU: operator_ref against the
dense R^T R + reg I formed entry by entry, tables_ref against hand-written expectations, every crafted layout against the property
it was built for, the exactness condition of every integer case, and -- once -- that the comparison helper of the bit-for-bit cases
fails when it is fed a subtly wrong result."""
import numpy as np
import pytest

import fused_op_ref as fr

ALL_LAYOUTS = sorted(fr.LAYOUTS)


def _toy():
    """40 rows, 2 levels, 10 unknowns (6 + 4): contiguous runs of cells, some rows without a level-0 cell, neighbours partly absent"""
    rs = np.random.RandomState(0)
    M = 10
    nbr = rs.randint(-1, M, (M, 27))
    rc = np.stack([np.repeat([0, 1, -1, 3, 5], [7, 9, 4, 12, 8]), np.repeat([6, 7, 9], [16, 16, 8])]).astype(np.int32)
    return rs, M, nbr, rc


@pytest.mark.parametrize('integral', [False, True])
def test_operator_ref_equals_the_dense_normal_matrix(integral):
    rs, M, nbr, rc = _toy()
    # (every unknown at most once per row: the 27 slots of a cell name different voxels)
    for j in range(M):
        nbr[j] = -1
        pick = rs.choice(27, 6, replace=False)
        nbr[j, pick] = rs.choice(M, 6, replace=False)
    rows = rs.randint(-2, 3, (2, 40, 27)).astype(np.float64) if integral else rs.randn(2, 40, 27)
    t = rs.randint(-3, 4, 40).astype(np.float64) if integral else rs.randn(40)
    x = rs.randint(-3, 4, M).astype(np.float64) if integral else rs.randn(M)
    reg = 0.5
    R = np.zeros((40, M))
    for d in range(2):
        for r in range(40):
            for s in range(27):
                if rc[d, r] >= 0 and nbr[rc[d, r], s] >= 0:
                    R[r, nbr[rc[d, r], s]] += rows[d, r, s]
    A = R.T @ R + reg * np.eye(M)
    out = fr.operator_ref(rows, rc, nbr, t, x, reg)
    k = out['scale']
    assert k == (2 if integral else 1) and out['y'].dtype == (np.int64 if integral else np.float64)
    np.testing.assert_allclose(out['y'] / k, A @ x, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out['b'], R.T @ t, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out['diag'] / k, np.diag(A), rtol=1e-12)
    np.testing.assert_allclose(out['mag'], np.abs(R).T @ (np.abs(R) @ np.abs(x)) + reg * np.abs(x), rtol=1e-12)
    np.testing.assert_allclose(out['mag_b'], np.abs(R).T @ np.abs(t), rtol=1e-12)
    assert out['nnz'] == np.count_nonzero(rows)
    # slots without an unknown do not enter: changing them changes nothing but the slot count
    rows2 = rows.copy()
    rows2[~fr.valid_slots(rc, nbr)] += 1.0
    out2 = fr.operator_ref(rows2, rc, nbr, t, x, reg)
    assert np.array_equal(out2['y'], out['y']) and np.array_equal(out2['diag'], out['diag'])


def test_tables_ref_on_hand_written_row_lists():
    # (a) 40 rows, two level-0 cells inside ONE level-1 cell: one workgroup, no partial blocks
    rc = np.stack([np.repeat([0, 1], [10, 30]), np.full(40, 2)])
    T = fr.tables_ref(rc, 3, 2)
    assert T['span'].tolist() == [[0, 10, 0], [9, 39, 39], [0, 0, 0]]
    assert T['item_begin'].tolist() == [0] + [40] * 8                       # no unit starts at or after row 32
    assert T['counts'].tolist() == [0, 0, 0, 0] and T['nblocks'] == 0 and T['n_multi'] == 0 and T['n_big'] == 0
    # (b) one level, two cells of 300 rows: each cell is ONE unit, hence inside one workgroup however long it is
    rc = np.repeat([0, 1], [300, 300])[None]
    T = fr.tables_ref(rc, 2, 1)
    assert T['item_begin'].tolist() == [0] + [300] * 9 + [600] * 15           # windows 1 .. 9 start at or before row 300
    assert T['span'].tolist() == [[0, 300], [299, 599], [0, 1]]
    assert T['counts'].tolist() == [0, 0, 0] and T['offsets'].tolist() == [0, 0, 0]
    # (c) a unit of 790 rows covers the whole windows of workgroups 1 and 2: they are empty, the unit belongs to workgroup 0, the
    # rows after it to workgroup 3 -- and the level-1 cell around them reaches into FOUR workgroups (block w = base + w)
    nb = np.full((5, 27), -1)
    nb[:, 13] = np.arange(5)
    rc = np.stack([np.repeat([0, 1, 2], [10, 790, 10]), np.repeat([3, 4], [5, 805])])
    T = fr.tables_ref(rc, 5, 2, nb)
    assert T['item_begin'].tolist() == [0] + [800] * 25 + [810] * 7
    assert T['span'].tolist() == [[0, 10, 800, 0, 5], [9, 799, 809, 4, 809], [0, 0, 3, 0, 0]]
    assert T['counts'].tolist() == [0, 0, 0, 0, 4, 0] and T['offsets'].tolist() == [0, 0, 0, 0, 0, 4]
    assert T['nblocks'] == 4 and T['multi'].tolist() == [4] and T['n_big'] == 0
    assert T['nbr32'][4].tolist() == [-1] * 13 + [4] + [-1] * 13 + [0, 5, 809, 0, 0]
    assert T['nbr32'][2, 27:].tolist() == [0 - 3, 800, 809, 0, 0]
    assert np.array_equal(T['nbrT'], nb.T)
    S = fr.layout_stats(rc, T=T)
    assert S['empty_wgs'] == 2 and S['units_longer_than'] == {32: 1, 256: 1, 288: 1} and S['max_wg_rows'] == 800


# what every layout was built for
def _has(S, name):
    c = S['counts']
    if name == 'sparse1':
        return S['max_wg_cells0'] > fr.STAGE0 and S['max_wg_cells1'] > fr.STAGE1 and S['wg_beyond_stage0'] > 0 and S['wg_beyond_stage1'] > 0
    if name == 'clumps':
        u = S['units_longer_than']
        return (u[32] >= 3 and u[256] >= 2 and u[288] >= 2 and S['empty_items'] >= 1 and S['empty_wgs'] >= 1
                and S['exchange_over_empty_item'] >= 1 and S['max_wg_rows'] > fr.RCAP)
    if name == 'blocks':
        return (any(2 <= v <= 4 for v in c) and 16 in c and 17 in c and any(25 <= v <= 32 for v in c) and any(33 <= v <= 120 for v in c)
                and any(121 <= v <= 128 for v in c) and any(v >= 257 for v in c) and S['cells_2_to_16'] % fr.GROUP != 0
                and S['empty_wgs'] == 0)
    if name == 'absent':
        return S['first_present'] == [-1, 0, 1, 2] and S['wg_first_row_without_c0'] >= 1
    if name == 'mixed' or name.startswith('depth'):
        return S['units_with_both_sets'] >= 1
    if name == 'segments2':
        return S['units_with_both_sets'] >= 1 and S['runs_without_cell'] == 2 and S['rows_total'] % 256 == 0
    if name.startswith('tiny'):
        return S['rows_total'] == int(name[4:])
    raise KeyError(name)


@pytest.mark.parametrize('name', ALL_LAYOUTS)
def test_every_layout_has_the_property_it_was_built_for(name):
    L = fr.layout(name)
    S = fr.layout_stats(L['row_cells'], L['row_sets'], L['tables'])
    assert _has(S, name), S
    assert L['row_cells'].shape[1] <= 70000 and L['layout'].depth == {'blocks': 5, 'depth1': 1, 'depth2': 2, 'depth6': 6}.get(name, 4)
    # the oracle hierarchy's own neighbour table says the same as the restated one
    off = fr.level_offsets(L['oh'].levels)
    for d, lv in enumerate(L['oh'].levels):
        assert np.array_equal(np.where(lv.nbr >= 0, lv.nbr + off[d], -1), L['nbr'][off[d]:off[d + 1]])


@pytest.mark.parametrize('name', ALL_LAYOUTS)
def test_integer_cases_stay_exact_in_fp32(name):
    """Every partial sum of the bit-for-bit cases is an integer below 2^24: mag bounds them all."""
    L = fr.layout(name)
    rows, t, xs = fr.integer_case(L['row_cells'], L['nbr'], seed=7)
    assert not rows[~fr.valid_slots(L['row_cells'], L['nbr'])].any() and set(np.unique(rows)) <= {-1, 0, 1}
    Rm = fr.rows_matrix(rows, L['row_cells'], L['nbr'], L['M'])
    for x in xs:
        for reg in (1.0, 0.5):
            out = fr.operator_ref(rows, L['row_cells'], L['nbr'], t, x, reg, Rm=Rm)
            assert out['y'].dtype == np.int64 and out['scale'] == (1 if reg == 1.0 else 2)
            assert out['mag'].max() < 2 ** 24 and out['mag_b'].max() < 2 ** 24 and out['diag'].max() < 2 ** 24
    # every row counts: it holds a non-zero slot at every level at which it has a cell with neighbours
    ok = fr.valid_slots(L['row_cells'], L['nbr']).any(2)
    assert (np.abs(rows).sum(2)[ok] > 0).mean() > 0.9


@pytest.mark.parametrize('name', ['blocks', 'clumps', 'absent'])
def test_the_exact_comparison_notices_one_lost_row_and_a_swapped_span(name):
    """The helper the GPU cases assert with, fed a "GPU" result that is wrong the way a sweep bug would make it: one row of a cell
    that spans several workgroups left out of that cell's block."""
    L = fr.layout(name)
    rc, nb, T = L['row_cells'], L['nbr'], L['tables']
    rows, t, xs = fr.integer_case(rc, nb, seed=7)
    ref = fr.operator_ref(rows, rc, nb, t, xs[0], 1.0)
    fr.compare_exact('y', ref['y'].astype(np.float32), ref['y'])                       # (the right answer passes)
    cell = int(T['multi'][-1])
    d = int(np.nonzero((rc == cell).any(1))[0][0])
    cand = np.nonzero((rc[d] == cell) & (np.abs(rows[d]).sum(1) > 0) & (t != 0))[0]
    wrong_rows = rows.copy()
    wrong_rows[d, cand[len(cand) // 2]] = 0
    wrong = fr.operator_ref(wrong_rows, rc, nb, t, xs[0], 1.0)
    hit = 0
    for k in ('b', 'diag', 'y'):
        try:
            fr.compare_exact(k, wrong[k].astype(np.float32), ref[k])
        except AssertionError:
            hit += 1
    assert hit >= 2, 'a lost row went unnoticed'
    with pytest.raises(AssertionError):
        fr.compare_exact('nnz', np.array([wrong['nnz']]), np.array([ref['nnz']]))
    swapped = T['span'][[1, 0, 2]]
    with pytest.raises(AssertionError):
        fr.compare_exact('span', swapped.reshape(-1), T['span'].reshape(-1))


def test_rounding_steps_and_gamma():
    L = fr.layout('clumps')
    m = fr.rounding_steps(L['tables'], L['nbr'], 4)
    assert m.min() == 27 * 4 + 35 + 1                                       # an unknown whose neighbour cells hold one row each
    assert m.max() == 27 * 4 + 35 + 1549 + 7                                # the coarsest cell holds all 1549 rows in 7 workgroups
    g = fr.gamma(m)
    assert (g > m * 2.0 ** -24).all() and abs(g.max() - 1699 * 2.0 ** -24) < 1e-7
