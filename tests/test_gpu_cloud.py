"""nksr_amd/cloud.py on the GPU against tests/cloud_ref.py (numpy / scipy cKDTree, float64): k nearest neighbours, radius counts, the
outlier masks, voxel downsampling (csrc/knn_query.hip k_knn_query_*, k_radius_count; csrc/cloud.hip k_voxel_reduce) and the preprocess_fn
plumbing.  The standard input, cloud A: 20 000 noisy sphere samples + 1 000 uniform stray points (cloud_ref.cloud_a).

Tolerances.  Distances: the kernels take fp32 differences of fp32 coordinates (<= 6e-8 relative each) and sum their squares in fp32,
<= ~2.5e-7 relative on the distance; rtol 1e-6 is a 4x margin.  Neighbour SETS are compared where the reference's k-th and (k+1)-th
distances differ by more than 1e-5 relative, counts where no neighbour lies within 1e-5 r of the radius (both far above the fp32
error; the reference alone excludes < 0.3 % of cloud A either way, at most 1 % may be excluded).  Voxel means: fp64 sums in another
order, rounded once to fp32: within one fp32 ulp of the rounded reference."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(None)
def _a():
    return R.cloud_a()


@functools.lru_cache(None)
def _index():
    from nksr_amd import cloud
    return cloud.CloudIndex(_gpu(_a()[0]))


@functools.lru_cache(None)
def _queries():
    return np.random.RandomState(3).uniform(-0.7, 0.7, (5000, 3)).astype(np.float32)


@functools.lru_cache(None)
def _ref_knn(mode):
    """33 (+1) reference neighbours once per kind of query: every k of the tests is a prefix"""
    x = _a()[0]
    if mode == 'query':
        return R.knn(x, 33, query=_queries())
    return R.knn(x, 33, exclude_self=mode == 'self_ex')


@functools.lru_cache(None)
def _ref_count(radius, exclude_self):
    return R.radius_count(_a()[0], radius, exclude_self=exclude_self)


def _check_knn(x, q, k, idx, dist, ref_j, ref_d):
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.shape == (len(q), k) and dist.shape == (len(q), k) and idx.dtype == np.int64 and dist.dtype == np.float32
    assert idx.min() >= 0 and idx.max() < len(x)
    assert (np.diff(dist, axis=1) >= 0).all()
    err = np.abs(dist - ref_d[:, :k]) / np.maximum(ref_d[:, :k], 1e-300)
    print('k=%d  max relative distance error %.3g' % (k, err[ref_d[:, :k] > 0].max() if (ref_d[:, :k] > 0).any() else 0.0))
    np.testing.assert_allclose(dist, ref_d[:, :k], rtol=1e-6, atol=0)
    # the indices are real: the distance to the points they name, recomputed in fp64
    re = np.linalg.norm(q.astype(np.float64)[:, None, :] - x.astype(np.float64)[idx], axis=2)
    np.testing.assert_allclose(dist, re, rtol=1e-6, atol=0)
    if ref_d.shape[1] > k:
        sure = (ref_d[:, k] - ref_d[:, k - 1]) > 1e-5 * ref_d[:, k]
        print('k=%d  rows compared as sets: %.4f' % (k, sure.mean()))
        assert sure.mean() >= 0.99
        assert (np.sort(idx[sure], axis=1) == np.sort(ref_j[sure, :k], axis=1)).all()


# ---- k nearest neighbours -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 8, 16, 32])
@pytest.mark.parametrize('mode', ['self', 'self_ex', 'query'])
def test_knn_matches_kdtree(mode, k):
    x = _a()[0]
    ref_j, ref_d = _ref_knn(mode)
    if mode == 'query':
        q = _queries()
        idx, dist = _index().knn(k, query=_gpu(q))
    else:
        q = x
        idx, dist = _index().knn(k, exclude_self=mode == 'self_ex')
        if mode == 'self':
            assert (dist[:, 0] == 0).all() and (idx[:, 0].cpu().numpy() == np.arange(len(x))).all()
        else:
            assert (idx.cpu().numpy() != np.arange(len(x))[:, None]).all()
    _check_knn(x, q, k, idx, dist, ref_j, ref_d)
    idx2, dist2 = _index().knn(k, query=_gpu(q)) if mode == 'query' else _index().knn(k, exclude_self=mode == 'self_ex')
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)


def test_knn_far_query_takes_the_coarse_grids():
    x = _a()[0]
    q = np.array([[50.0, 50.0, 50.0], [0.0, 0.0, 0.0], [-30.0, 2.0, 1.0], [0.45, 0.0, 0.0]], np.float32)
    for k in (1, 8):
        idx, dist = _index().knn(k, query=_gpu(q))
        ref_j, ref_d = R.knn(x, k, query=q)
        _check_knn(x, q, k, idx, dist, ref_j, ref_d[:, :k])
        sure = (ref_d[:, k] - ref_d[:, k - 1]) > 1e-5 * ref_d[:, k]
        assert (np.sort(idx.cpu().numpy()[sure], axis=1) == np.sort(ref_j[sure, :k], axis=1)).all()


@functools.lru_cache(None)
def _dup():
    """600 random points with 40 exact copies among them, 200 queries near the cloud, and the CloudIndex over the points"""
    from nksr_amd import cloud
    rs = np.random.RandomState(11)
    x = rs.rand(600, 3).astype(np.float32)
    x = np.concatenate([x, x[rs.randint(0, 600, 40)]])
    q = (x[rs.randint(0, 640, 200)] + 0.05 * rs.randn(200, 3)).astype(np.float32)
    return x, q, cloud.CloudIndex(_gpu(x))


@pytest.mark.parametrize('mode,k', [(m, k) for m in ('query', 'self') for k in (1, 8, 9, 17, 32)] + [('self_ex', 32)])
def test_one_level_pyramid_finds_what_the_octree_finds(mode, k):
    """nksr_knn_query_pyramid on the octree and on the same grid as a pyramid of ONE level (what the coarse rounds run): where both
    answer, the k smallest squared distances are one multiset, computed by the same knn_d2 -- bit for bit equal.  Both against an fp64
    brute force at the 1e-5 relative tolerance of this file; self_ex at k = 32 is the 33-slot list."""
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import PointPyramid
    x, q, ci = _dup()
    pg, ex = ci.pg, mode == 'self_ex'
    one = PointPyramid(pg, max_levels=1)
    assert one.levels == 1 and one.struct.levels == 1 and ci.pyramid.levels > 1
    qg = _gpu(q) if mode == 'query' else None
    qs = qg if mode == 'query' else pg.xyz                 # (a self-query runs in the grid's order)
    nq = qs.shape[0]

    def run(pyr):
        idx = torch.zeros((nq, k), dtype=torch.int32, device=DEV)
        d2 = torch.zeros((nq, k), dtype=torch.float32, device=DEV)
        valid = torch.zeros(nq, dtype=torch.int32, device=DEV)
        call('nksr_knn_query_pyramid', pyr.struct, ci.n, ptr(qg), nq, k, int(ex), None, 4, ptr(idx), ptr(d2), ptr(valid), stream())
        return idx.long(), d2, valid > 0
    ia, da, va = run(ci.pyramid)
    ib, db, vb = run(one)
    both = va & vb
    print('%s k=%d  valid: octree %d, one level %d of %d' % (mode, k, int(va.sum()), int(vb.sum()), nq))
    assert int(both.sum()) >= nq // 2
    assert torch.equal(da[both], db[both])
    exact = 'donot_use_mm_for_euclid_dist'                 # (the matrix-product form leaves ~1e-8 where two points coincide)
    full = torch.cdist(qs.double(), pg.xyz.double(), compute_mode=exact)
    if ex:
        full.fill_diagonal_(float('inf'))
    ref = full.topk(k, dim=1, largest=False).values
    for idx, d2, v in ((ia, da, va), (ib, db, vb)):
        torch.testing.assert_close(d2[v].double().sqrt(), ref[v], rtol=1e-5, atol=0)
        torch.testing.assert_close(torch.gather(full, 1, idx)[v], ref[v], rtol=1e-5, atol=0)    # the indices name points at those distances
    # a row the single level does not reach is answered by the rounds: knn() raises if one is left, and agrees with the brute force
    idx, dist = ci.knn(k, query=qg, exclude_self=ex)
    back = torch.cdist((qg if mode == 'query' else ci.xyz).double(), ci.xyz.double(), compute_mode=exact)
    if ex:
        back.fill_diagonal_(float('inf'))
    ref = back.topk(k, dim=1, largest=False).values
    torch.testing.assert_close(dist.double(), ref, rtol=1e-5, atol=0)
    torch.testing.assert_close(torch.gather(back, 1, idx), ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize('k', [8, 32])
def test_knn_duplicates_stay_when_the_point_itself_is_excluded(k):
    from nksr_amd import cloud
    x = np.concatenate([np.tile(np.array([[0.1, 0.2, 0.3]], np.float32), (64, 1)), np.random.RandomState(5).rand(100, 3).astype(np.float32)])
    idx, dist = cloud.CloudIndex(_gpu(x)).knn(k, exclude_self=True)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert (dist[:64] == 0).all() and (idx[:64] < 64).all()                          # copies come back at distance 0 ...
    assert (idx != np.arange(len(x))[:, None]).all()                                  # ... never the point itself
    assert all(len(set(row)) == k for row in idx)
    ref_j, ref_d = R.knn(x, k, exclude_self=True)
    np.testing.assert_allclose(dist, ref_d[:, :k], rtol=1e-6, atol=0)


def test_knn_small_clouds_and_errors():
    from nksr_amd import cloud
    one = cloud.CloudIndex(_gpu(np.array([[0.5, -0.25, 2.0]], np.float32)))
    idx, dist = one.knn(1)
    assert idx.tolist() == [[0]] and dist.tolist() == [[0.0]]
    idx, dist = one.knn(1, query=_gpu(np.array([[0.5, -0.25, 0.0], [4.5, -0.25, 5.0]], np.float32)))
    assert idx.tolist() == [[0], [0]] and dist.tolist() == [[2.0], [5.0]]
    with pytest.raises(ValueError):
        one.knn(2)
    with pytest.raises(ValueError):
        one.knn(1, exclude_self=True)
    x = np.random.RandomState(8).rand(8, 3).astype(np.float32)                      # N = k
    q = np.array([[0.5, 0.5, 0.5], [9.0, -3.0, 0.0]], np.float32)
    ci = cloud.CloudIndex(_gpu(x))
    for query in (None, q):
        idx, dist = ci.knn(8, query=None if query is None else _gpu(query))
        ref_j, ref_d = R.knn(x, 8, query=query)
        _check_knn(x, x if query is None else query, 8, idx, dist, ref_j, ref_d)
        assert (np.sort(idx.cpu().numpy(), axis=1) == np.arange(8)).all()
    idx, dist = ci.knn(7, exclude_self=True)
    np.testing.assert_allclose(dist.cpu().numpy(), R.knn(x, 7, exclude_self=True)[1][:, :7], rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        ci.knn(8, exclude_self=True)
    with pytest.raises(ValueError):
        _index().knn(33)
    with pytest.raises(ValueError):
        _index().knn(0)
    with pytest.raises(RuntimeError):
        cloud.CloudIndex(torch.from_numpy(x))
    with pytest.raises(RuntimeError):
        _index().knn(4, query=torch.from_numpy(q))
    with pytest.raises(RuntimeError):
        cloud.CloudIndex(_gpu(np.array([[0.0, np.nan, 0.0], [1.0, 0.0, 0.0]], np.float32)))


# ---- radius count and the radius mask -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', [None, 8])
@pytest.mark.parametrize('radius', [0.03, 0.05])
def test_radius_count_matches_kdtree(radius, cap):
    for ex in (False, True):
        ref, sure = _ref_count(radius, ex)
        cnt = _index().radius_count(radius, cap=cap, exclude_self=ex)
        assert cnt.dtype == torch.int32 and cnt.shape == (len(ref),)
        assert torch.equal(cnt, _index().radius_count(radius, cap=cap, exclude_self=ex))
        cnt = cnt.cpu().numpy()
        print('r=%g  points compared: %.4f  differing inside the band: %d' % (radius, sure.mean(), (cnt != (ref if cap is None else np.minimum(ref, cap)))[~sure].sum()))
        assert sure.mean() >= 0.99
        assert (cnt[sure] == (ref if cap is None else np.minimum(ref, cap))[sure]).all()
        if cap is not None:
            assert cnt.max() <= cap


def test_radius_count_of_queries():
    q = np.concatenate([_queries()[:2000], np.array([[50.0, 50.0, 50.0]], np.float32)])
    ref, sure = R.radius_count(_a()[0], 0.05, query=q)
    cnt = _index().radius_count(0.05, query=_gpu(q)).cpu().numpy()
    assert sure.mean() >= 0.99 and (cnt[sure] == ref[sure]).all() and cnt[-1] == 0


def test_radius_outlier_mask():
    from nksr_amd import cloud
    x = _a()[0]
    ref, sure = _ref_count(0.05, True)
    keep = cloud.radius_outlier_mask(_gpu(x), 0.05, 8)
    assert keep.dtype == torch.bool and keep.shape == (len(x),)
    keep = keep.cpu().numpy()
    assert (keep[sure] == (ref >= 8)[sure]).all()
    print('removed: %d of the 1000 stray points, %d of the 20000 sphere points' % ((~keep[20000:]).sum(), (~keep[:20000]).sum()))
    assert (~keep[20000:]).sum() >= 850 and (~keep[:20000]).sum() <= 100
    assert cloud.radius_outlier_mask(_gpu(x), 0.05, 0).all()


# ---- statistical mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('std_ratio', [1.0, 2.0])
def test_statistical_outlier_mask(std_ratio):
    from nksr_amd import cloud
    x = _a()[0]
    ref_mask, ref_m, thr = R.statistical_outlier(x, 16, std_ratio)
    m = _index().mean_knn_distance(16)
    assert m.dtype == torch.float32
    np.testing.assert_allclose(m.cpu().numpy(), ref_m, rtol=1e-6, atol=0)
    keep = cloud.statistical_outlier_mask(_gpu(x), 16, std_ratio).cpu().numpy()
    clear = np.abs(ref_m - thr) > 1e-4 * thr
    assert (keep[clear] == ref_mask[clear]).all() and clear.mean() >= 0.99


# ---- voxel downsampling -------------------------------------------------------------------------------------------------------------
def _within_one_ulp(got, ref64):
    ref32 = ref64.astype(np.float32)
    return (np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)).all()


def _check_nearest(x, ref, index, inverse_rows=None):
    """index[v] is a point of voxel v at minimal distance to the voxel's (fp64) centroid; the two fp64 centroids differ by summation
    order only, ~1e-16, hence 1e-12"""
    assert (ref['inverse'][index] == np.arange(len(index))).all()
    d = np.linalg.norm(x.astype(np.float64) - ref['xyz'][ref['inverse']], axis=1)
    dmin = np.full(len(index), np.inf)
    np.minimum.at(dmin, ref['inverse'], d)
    assert (d[index] <= dmin + 1e-12).all()


@functools.lru_cache(None)
def _color():
    return np.random.RandomState(4).rand(21000, 3).astype(np.float32)


@pytest.mark.parametrize('voxel_size', [0.02, 0.05])
def test_voxel_downsample_mean(voxel_size):
    from nksr_amd import cloud
    x, nrm = _a()
    col = _color()
    ref = R.voxel_downsample(x, voxel_size, [nrm, col])
    r = cloud.voxel_downsample(_gpu(x), voxel_size, normal=_gpu(nrm), color=_gpu(col))
    assert len(r) == len(ref['count']) and r.sensor is None and r.index is None
    assert r.inverse.dtype == torch.int64 and (r.inverse.cpu().numpy() == ref['inverse']).all()      # same partition, rows in key order
    assert r.count.dtype == torch.int32 and (r.count.cpu().numpy() == ref['count']).all()
    assert _within_one_ulp(r.xyz.cpu().numpy(), ref['xyz']) and _within_one_ulp(r.color.cpu().numpy(), ref['attrs'][1])
    n = r.normal.cpu().numpy()
    np.testing.assert_allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=2e-7)
    # the fp32 mean is within 6e-8 relative per component of the fp64 one, scaling to unit length (fp64) and rounding add as much again
    np.testing.assert_allclose(n, R.unit_normals(ref['attrs'][0], nrm[ref['first']]), atol=5e-7, rtol=0)
    r2 = cloud.voxel_downsample(_gpu(x), voxel_size, normal=_gpu(nrm), color=_gpu(col))
    for a, b in ((r.xyz, r2.xyz), (r.normal, r2.normal), (r.color, r2.color), (r.count, r2.count), (r.inverse, r2.inverse)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('voxel_size', [0.02, 0.05])
def test_voxel_downsample_nearest(voxel_size):
    from nksr_amd import cloud
    x, nrm = _a()
    col = _color()
    ref = R.voxel_downsample(x, voxel_size)
    r = cloud.voxel_downsample(_gpu(x), voxel_size, normal=_gpu(nrm), color=_gpu(col), reduce='nearest')
    index = r.index.cpu().numpy()
    assert r.index.dtype == torch.int64 and (r.inverse.cpu().numpy() == ref['inverse']).all() and (r.count.cpu().numpy() == ref['count']).all()
    _check_nearest(x, ref, index)
    assert (r.xyz.cpu().numpy() == x[index]).all() and (r.normal.cpu().numpy() == nrm[index]).all() and (r.color.cpu().numpy() == col[index]).all()
    assert torch.equal(r.index, cloud.voxel_downsample(_gpu(x), voxel_size, reduce='nearest').index)


@pytest.mark.parametrize('group', [1, 7, 64])
def test_voxel_reduce_with_every_group_size(group):
    """voxels per wavefront: chosen from the voxel count in production (1 or 2 at these sizes); every mapping gives the same means"""
    from nksr_amd import cloud
    x, nrm = _a()
    xg, ng = _gpu(x), _gpu(nrm)
    ref = R.voxel_downsample(x, 0.02, [nrm])
    order, keys, start, end = cloud.voxel_runs(xg, 0.02)
    mean, amean, count, near = cloud.voxel_reduce(order, start, end, xg, ng, nearest=True, group=group)
    assert (count.cpu().numpy() == ref['count']).all()
    assert _within_one_ulp(mean.cpu().numpy(), ref['xyz']) and _within_one_ulp(amean.cpu().numpy(), ref['attrs'][0])
    pos = near.cpu().numpy()
    assert (pos >= start.cpu().numpy()).all() and (pos < end.cpu().numpy()).all()
    _check_nearest(x, ref, order.cpu().numpy()[pos])
    again = cloud.voxel_reduce(order, start, end, xg, ng, nearest=True, group=group)
    assert all(torch.equal(a, b) for a, b in zip((mean, amean, count, near), again))


def test_voxel_downsample_edge_shapes():
    from nksr_amd import cloud
    # N = 0 and N = 1
    r = cloud.voxel_downsample(torch.zeros((0, 3), device=DEV), 0.1, normal=torch.zeros((0, 3), device=DEV), reduce='nearest')
    assert len(r) == 0 and r.xyz.shape == (0, 3) and r.normal.shape == (0, 3) and r.count.numel() == 0 and r.inverse.numel() == 0 and r.index.numel() == 0
    p = np.array([[0.3, -0.7, 0.2]], np.float32)
    r = cloud.voxel_downsample(_gpu(p), 0.1, normal=_gpu(np.array([[0.0, 3.0, 4.0]], np.float32)), reduce='mean')
    assert (r.xyz.cpu().numpy() == p).all() and r.count.tolist() == [1] and r.inverse.tolist() == [0]
    np.testing.assert_allclose(r.normal.cpu().numpy(), [[0.0, 0.6, 0.8]], atol=1e-7)
    # 5000 points in one voxel (a run far longer than a wavefront) next to three lone ones; four copies of one point tie
    rs = np.random.RandomState(6)
    x = np.concatenate([0.05 + 0.9 * rs.rand(5000, 3), [[1.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, 2.5, 0.5]]]).astype(np.float32)
    att = rs.randn(len(x), 5).astype(np.float32)
    ref = R.voxel_downsample(x, 1.0, [att])
    assert sorted(ref['count'].tolist()) == [1, 1, 1, 5000]
    for reduce in ('mean', 'nearest'):
        r = cloud.voxel_downsample(_gpu(x), 1.0, color=_gpu(att), reduce=reduce)
        assert (r.inverse.cpu().numpy() == ref['inverse']).all() and (r.count.cpu().numpy() == ref['count']).all()
        if reduce == 'mean':
            assert _within_one_ulp(r.xyz.cpu().numpy(), ref['xyz']) and _within_one_ulp(r.color.cpu().numpy(), ref['attrs'][0])
        else:
            _check_nearest(x, ref, r.index.cpu().numpy())
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (4, 1))
    r = cloud.voxel_downsample(_gpu(np.concatenate([x[:10], dup])), 1.0, reduce='nearest')
    r4 = cloud.voxel_downsample(_gpu(dup), 1.0, reduce='nearest')
    assert r4.index.tolist() == [0] and r4.count.tolist() == [4] and len(r) == 1           # all four at distance 0: the lowest index
    # opposing normals cancel: the normal of the voxel's lowest-index point
    r = cloud.voxel_downsample(_gpu(dup[:2]), 1.0, normal=_gpu(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], np.float32)))
    assert r.normal.tolist() == [[0.0, 0.0, 1.0]]
    # a voxel so small that every point is alone: the output is the input, in key order
    x = _a()[0][:3000]
    ref = R.voxel_downsample(x, 1e-5)
    assert (ref['count'] == 1).all()
    r = cloud.voxel_downsample(_gpu(x), 1e-5)
    assert (r.inverse.cpu().numpy() == ref['inverse']).all() and (r.xyz.cpu().numpy()[ref['inverse']] == x).all() and (r.count == 1).all()
    # points straddling the origin on all three axes (floor, not truncation)
    x = np.random.RandomState(7).uniform(-0.05, 0.05, (2000, 3)).astype(np.float32)
    ref = R.voxel_downsample(x, 0.02)
    assert (ref['ijk'].min(0) < 0).all() and (ref['ijk'].max(0) >= 0).all()
    r = cloud.voxel_downsample(_gpu(x), 0.02)
    assert (r.inverse.cpu().numpy() == ref['inverse']).all() and (r.count.cpu().numpy() == ref['count']).all()
    assert _within_one_ulp(r.xyz.cpu().numpy(), ref['xyz'])
    # float64 and non-contiguous inputs: the same result as float32 contiguous
    wide = torch.zeros((len(x), 6), dtype=torch.float64, device=DEV)
    wide[:, 1:4] = _gpu(x).double()
    r2 = cloud.voxel_downsample(wide[:, 1:4], 0.02, color=wide[:, 1:4])
    assert not wide[:, 1:4].is_contiguous() and torch.equal(r2.xyz, r.xyz) and torch.equal(r2.inverse, r.inverse) and torch.equal(r2.color, r.xyz)
    idx, dist = _index().knn(8, query=wide[:500, 1:4])
    idx2, dist2 = _index().knn(8, query=_gpu(x[:500]))
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)
    with pytest.raises(ValueError):
        cloud.voxel_downsample(_gpu(x), 0.02, reduce='median')
    with pytest.raises(RuntimeError):
        cloud.voxel_downsample(_gpu(x), 1e-9)                      # |x| / voxel_size past 2^20


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def test_composed_preprocess_fn_equals_the_steps_by_hand():
    import nksr
    x, nrm = _a()
    xg, ng = _gpu(x), _gpu(nrm)
    fn = nksr.compose_preprocess_fns(nksr.get_radius_outlier_preprocess_fn(0.05, 8), nksr.get_voxel_downsample_preprocess_fn(0.01))
    rec = nksr.Reconstructor(torch.device(DEV))
    f1 = rec.reconstruct(xg, ng, preprocess_fn=fn, voxel_size=0.05)
    keep = nksr.cloud.radius_outlier_mask(xg, 0.05, 8)
    ds = nksr.cloud.voxel_downsample(xg[keep], 0.01, normal=ng[keep])
    assert 1000 < len(ds) < int(keep.sum())
    f2 = rec.reconstruct(ds.xyz, ds.normal, voxel_size=0.05)
    pts = _gpu(np.random.RandomState(9).uniform(-0.5, 0.5, (1000, 3)).astype(np.float32))
    assert torch.equal(f1.evaluate_f(pts).value, f2.evaluate_f(pts).value)
    x2, n2, s2 = fn(xg, None, None)
    assert n2 is None and s2 is None and torch.equal(x2, ds.xyz)
    # filters keep the input order and carry every slot
    x3, n3, s3 = nksr.get_statistical_outlier_preprocess_fn(16, 2.0)(xg, ng, xg * 2)
    keep3 = nksr.cloud.statistical_outlier_mask(xg, 16, 2.0)
    assert torch.equal(x3, xg[keep3]) and torch.equal(n3, ng[keep3]) and torch.equal(s3, xg[keep3] * 2)


def test_composed_preprocess_fn_in_front_of_normal_estimation():
    import nksr
    x = _a()[0]
    xg = _gpu(x)
    sensor = torch.zeros_like(xg)                              # scanner at the centre of the sphere
    fn = nksr.compose_preprocess_fns(nksr.get_radius_outlier_preprocess_fn(0.05, 8), nksr.get_voxel_downsample_preprocess_fn(0.01),
                                     nksr.get_estimate_normal_preprocess_fn(64, 85.0))
    x2, n2, s2 = fn(xg, None, sensor)
    assert s2 is None and x2.shape == n2.shape and x2.shape[0] > 5000
    x2, n2 = x2.cpu().numpy(), n2.cpu().numpy()
    np.testing.assert_allclose(np.linalg.norm(n2, axis=1), 1.0, atol=1e-4)
    assert ((-x2 * n2).sum(1) > 0).all()                       # every normal faces the sensor
    # a stray point that survives has 8 neighbours within 0.05 -- sphere samples, the strays being 0.3 to such a ball -- so what is left
    # lies within 0.05 + the noise of the surface
    assert np.abs(np.linalg.norm(x2, axis=1) - 0.45).max() < 0.07
