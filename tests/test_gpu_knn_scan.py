"""The shared candidate scan of the 27-cell kernels (csrc/knn_dev.h: knn_cells27, knn_scan4 -- groups of four, then a tail) through its
three users: nksr_radius_count (knn_query.hip), nksr_knn_query_pyramid (knn_scan in knn_topk_dev.h) and nksr_icp_accumulate
(register.hip), at the smallest shapes where a group-of-four loop can go wrong.

The cloud: 76 points on the dyadic lattice (multiples of 1/64) in the 27 cells of size 0.25 around the origin, the cells holding
0, 1, 2, 3, 4, 5, 7, 8 and 9 points (an empty cell, a tail only, groups only, groups plus a tail; asserted below).  Every coordinate
difference is a multiple of 1/64 below 2 and every squared distance a multiple of 1/4096 below 12: exact in fp32, so a float64 brute
force is the exact answer and everything is compared with ==.  The cell (1, 1, 1) is a corner of the occupied block: 19 of the 27
cells around a query there do not exist.  Two pairs lie at distance exactly 0.25 and 0.125 (they count), one point is stored twice.

Neighbour indices are compared, as sets, on the rows whose k-th and (k+1)-th brute-force distances differ; the share of rows left out
is printed and at most 10 % (on this cloud the brute force alone leaves out 4, 5, 5 and 10 of the 185 rows at k = 1, 4, 5 and 9, at
most 5.4 %: lattice distances repeat)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CELL = 0.25
# points per cell, cell j = (j // 9 - 1, (j // 3) % 3 - 1, j % 3 - 1): the order knn_cells27 walks them in
POPS = [3, 0, 7, 1, 4, 0, 8, 2, 0,
        5, 0, 1, 0, 9, 4, 2, 0, 3,
        0, 7, 1, 8, 0, 2, 0, 4, 5]


@functools.lru_cache(None)
def cloud():
    """float32 [76, 3] in a shuffled (caller) order"""
    rs = np.random.RandomState(11)
    pts = []
    for j, pop in enumerate(POPS):
        c = np.array([j // 9 - 1, (j // 3) % 3 - 1, j % 3 - 1])
        sub = [tuple(int(v) for v in s) for s in np.stack(np.unravel_index(rs.permutation(16 ** 3), (16, 16, 16)), 1)]
        fixed = {13: [(0, 0, 0), (0, 0, 8)], 14: [(0, 0, 0)]}.get(j, [])     # (0,0,0), (0,0,1/8), (0,0,1/4): pairs at exactly 1/8 and 1/4
        chosen = fixed + [s for s in sub if s not in fixed][:pop - len(fixed)]
        if j == 0:
            chosen[-1] = chosen[0]                                           # one point stored twice
        pts += [(c * 16 + np.array(s)) / 64.0 for s in chosen]
    x = np.array(pts, dtype=np.float64)
    x = x[rs.permutation(len(x))]
    assert (x * 64 == np.round(x * 64)).all() and np.abs(x).max() <= 1.0
    return x.astype(np.float32)


@functools.lru_cache(None)
def queries():
    """separate queries, float32 [33 + 2, 3]: lattice points in and around the block (one in every cell, the empty ones included, and
    six more), then two with nothing within 0.25 -- the last two are not given to the k-NN search of a single grid"""
    rs = np.random.RandomState(12)
    cells = np.array([[j // 9 - 1, (j // 3) % 3 - 1, j % 3 - 1] for j in range(27)])
    q = (cells * 16 + rs.randint(0, 16, (27, 3))) / 64.0
    more = rs.randint(-24, 40, (6, 3)) / 64.0
    far = np.array([[63, -63, 32], [-64, 40, 40]]) / 64.0
    return np.concatenate([q, more, far]).astype(np.float32)


def cell_index(x):
    return np.floor(x.astype(np.float64) / CELL).astype(np.int64)


def d2_matrix(q, x):
    e = q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]
    return (e * e).sum(2)


def test_layout_of_the_cloud():
    """(runs without a GPU call: the generator cannot silently lose a case)"""
    x, q = cloud(), queries()
    c = cell_index(x)
    assert c.min() == -1 and c.max() == 1 and len(x) == sum(POPS) == 76
    pops = np.bincount((c[:, 0] + 1) * 9 + (c[:, 1] + 1) * 3 + c[:, 2] + 1, minlength=27)
    assert pops.tolist() == POPS and set(POPS) == {0, 1, 2, 3, 4, 5, 7, 8, 9}
    assert POPS[26] > 0 and POPS[13] == 9                       # the corner cell (1, 1, 1) holds queries; the centre cell the most
    d2 = d2_matrix(x, x)
    assert (d2 == 0.25 ** 2).any() and (d2 == 0.125 ** 2).any()                  # pairs at exactly r
    assert (np.triu(d2 == 0, 1)).sum() == 1                                      # one duplicated point
    assert (d2.astype(np.float32).astype(np.float64) == d2).all()                # every squared distance is an fp32 number
    qc = cell_index(q[:27])
    assert sorted(map(tuple, qc)) == sorted((j // 9 - 1, (j // 3) % 3 - 1, j % 3 - 1) for j in range(27))
    assert (d2_matrix(q[-2:], x).min(1) > 0.25 ** 2).all()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(None)
def grid():
    from nksr_amd.neighbours import PointGrid
    g = PointGrid(_gpu(cloud()), CELL)
    assert g.inv_cell == 4.0
    return g


@functools.lru_cache(None)
def perm():
    return grid().perm.cpu().numpy()


# ---- nksr_radius_count --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [0.25, 0.125])
@pytest.mark.parametrize('mode', ['self', 'self_ex', 'query'])
def test_radius_count(radius, mode):
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import _grid_args
    g, x = grid(), cloud()
    q = queries() if mode == 'query' else x[perm()]                   # (query NULL: the cloud in the grid's order, row i = sorted point i)
    within = d2_matrix(q, x) <= radius * radius
    want = within.sum(1) - (mode == 'self_ex')
    assert want.max() >= 4 and (want == 0).any() == (mode != 'self')
    for cap in (None, int(want.max()), int(want.max()) - 1, 1):
        cnt = torch.full((len(q),), -7, dtype=torch.int32, device=DEV)
        call('nksr_radius_count', ptr(g.xyz), len(x), *_grid_args(g), ptr(_gpu(q)) if mode == 'query' else None, len(q), radius,
             cap or 0, int(mode == 'self_ex'), None, ptr(cnt), stream())
        ref = want if cap is None else np.minimum(want, cap)
        got = cnt.cpu().numpy()
        print('radius %g %s cap %s: counts up to %d, %d rows at the cap' % (radius, mode, cap, want.max(), 0 if cap is None else (want >= cap).sum()))
        assert np.array_equal(got, ref), (cap, got, ref)


# ---- nksr_knn_query_pyramid ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def pyramid(levels, leaf):
    from nksr_amd.neighbours import PointPyramid
    p = PointPyramid(grid(), leaf=leaf, max_levels=levels)
    assert (p.levels == 1) == (levels == 1)
    return p


@functools.lru_cache(None)
def brute(mode):
    """(d2 [Q, 76] ascending, caller index [Q, 76]) of the rows of `mode`; self_ex: the query's own point moved to the end"""
    x = cloud()
    q = queries()[:-2] if mode == 'query' else x[perm()]
    d2 = d2_matrix(q, x)
    if mode == 'self_ex':
        d2[np.arange(len(q)), perm()] = np.inf
    order = np.argsort(d2, axis=1, kind='stable')
    return np.take_along_axis(d2, order, 1), order


RINGS = 4
# leaf below (1) and above (16) every cell's population on the single grid; on the octree 2 (descends to the finest cells) and the default
@pytest.mark.parametrize('levels,leaf', [(1, 1), (1, 16), (8, 2), (8, 0)])
@pytest.mark.parametrize('k', [1, 4, 5, 9])
def test_knn_query(k, levels, leaf):
    from nksr_amd._lib import call, ptr, stream
    x, P = cloud(), pyramid(levels, leaf)
    left_out = rows = 0
    for mode in ('self', 'self_ex', 'query'):
        want_d2, want_idx = brute(mode)
        nq = len(want_d2)
        assert (want_d2[:, k - 1] <= (RINGS * CELL) ** 2).all()             # within reach of RINGS rings of the finest grid: every row valid
        qs = _gpu(queries()[:-2]) if mode == 'query' else None
        idx = torch.full((nq, k), -7, dtype=torch.int32, device=DEV)
        d2 = torch.full((nq, k), -7.0, dtype=torch.float32, device=DEV)
        valid = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
        call('nksr_knn_query_pyramid', P.struct, len(x), ptr(qs), nq, k, int(mode == 'self_ex'), None, RINGS, ptr(idx), ptr(d2), ptr(valid),
             stream())
        assert (valid.cpu().numpy() == 1).all()
        assert np.array_equal(d2.cpu().numpy().astype(np.float64), want_d2[:, :k])
        got = np.sort(perm()[idx.cpu().numpy()], axis=1)
        sure = want_d2[:, k - 1] < want_d2[:, k]
        assert np.array_equal(got[sure], np.sort(want_idx[:, :k], axis=1)[sure])
        left_out += int((~sure).sum())
        rows += nq
    print('k=%d levels=%d leaf=%d: %d of %d rows left out of the index comparison (k-th distance tied): %.1f %%' % (
        k, P.levels, leaf, left_out, rows, 100.0 * left_out / rows))
    assert left_out <= 0.10 * rows


# ---- nksr_icp_accumulate: the correspondences ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', [0, 1])
def test_icp_correspondences(method):
    from nksr_amd import register
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import _grid_args
    g, x = grid(), cloud()
    dup = np.argwhere(np.triu(d2_matrix(x, x) == 0, 1))[0]
    edge = np.array([[-32, -4, 18], [-20, -2, -8]], dtype=np.float32) / 64      # nearest point(s) at exactly 0.25: one, and two of them
    src = np.concatenate([queries(), x[dup[1]][None], edge, x[::5]])            # the queries, the duplicated point (by its higher index), cloud points
    d2 = d2_matrix(src, x)
    d2[d2 > CELL * CELL] = np.inf
    want = np.where(np.isfinite(d2.min(1)), np.argmin(d2, axis=1), -1)           # argmin: the lowest caller index among equals
    assert (want == -1).sum() >= 2 and want[len(queries())] == dup[0]
    at_r = (d2[len(queries()) + 1:len(queries()) + 3] == CELL * CELL).sum(1)
    assert at_r.tolist() == [1, 2] and (d2.min(1)[len(queries()) + 1:len(queries()) + 3] == CELL * CELL).all()
    assert ((d2 == d2.min(1, keepdims=True)).sum(1)[want >= 0] > 1).any()        # ties that the caller index decides
    nrm = np.random.RandomState(13).normal(size=(len(x), 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    normal = _gpu(nrm)[g.perm].contiguous()
    pose = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0], dtype=torch.float64, device=DEV)      # identity [12] + centre [3]
    nrows = (len(src) + register.BLOCK - 1) // register.BLOCK
    corr = torch.full((len(src),), -7, dtype=torch.int64, device=DEV)
    partials = torch.empty((nrows, register.FIELDS), dtype=torch.float64, device=DEV)
    call('nksr_icp_accumulate', ptr(g.xyz), len(x), *_grid_args(g), ptr(g.perm), ptr(normal) if method else None, ptr(_gpu(src)), len(src),
         pose.data_ptr(), pose.data_ptr() + 12 * 8, CELL, method, ptr(corr), ptr(partials), stream())
    got = corr.cpu().numpy()
    print('method %d: %d of %d source points without a correspondence' % (method, (want < 0).sum(), len(src)))
    assert np.array_equal(got, want)
