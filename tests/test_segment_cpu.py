"""Segmentation without a GPU: the restatement (tests/segment_ref.py) on hand cases, the conditions on the inputs that
tests/test_gpu_segment.py relies on -- asserted here on the restatement alone, before a GPU is involved --, the host-side functions of
nksr_amd/segment.py against it, and the C entry points rejecting bad arguments before any launch."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import segment_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on hand cases -------------------------------------------------------------------------------------------------------
def test_two_points_exactly_eps_apart_are_neighbours():
    k = np.array([[0, 0, 0], [3, 4, 0]])                    # 5 units apart
    out = S.dbscan_lattice(k, 5, 2)
    assert out['at_radius'] == 1 and out['core'].all() and out['labels'].tolist() == [0, 0] and out['sizes'].tolist() == [2]
    out = S.dbscan_lattice(k, 4, 2)
    assert not out['core'].any() and out['labels'].tolist() == [-1, -1] and out['n_clusters'] == 0
    x = S.lattice_xyz(k)
    assert S.dbscan_real(x, 5 * S.UNIT, 2)['labels'].tolist() == [0, 0]             # (3, 4, 5) * 2^-10: exact in float64 too


def test_chain_is_one_cluster_and_its_ends_are_border_points():
    k = np.stack([np.arange(10) * 2, np.zeros(10, int), np.zeros(10, int)], axis=1)
    out = S.dbscan_lattice(k, 2, 3)                         # inner points: themselves + two; the ends: themselves + one
    assert out['core'].tolist() == [False] + [True] * 8 + [False]
    assert out['labels'].tolist() == [0] * 10 and out['border'].sum() == 2 and out['sizes'].tolist() == [10]
    out = S.dbscan_lattice(k[[0, 1, 2, 3, 5, 6, 7, 8]], 2, 2)                      # a gap of 4 units: two clusters
    assert out['labels'].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]


def test_border_point_between_two_clusters_takes_the_lower_label():
    # two dense groups of four either side of a lone point that is within reach of one point of each and has no third neighbour
    left = [[-4, 0, 0], [-4, 1, 0], [-4, -1, 0], [-5, 0, 0]]
    right = [[4, 0, 0], [4, 1, 0], [4, -1, 0], [5, 0, 0]]
    for k in (right + [[0, 0, 0]] + left, left + [[0, 0, 0]] + right):
        out = S.dbscan_lattice(np.array(k), 4, 4)
        assert out['core'].tolist() == [True] * 4 + [False] + [True] * 4
        assert out['labels'].tolist() == [0] * 5 + [1] * 4 and out['sizes'].tolist() == [5, 4]
    # the label order follows the smallest CORE index: a border point in front of everything does not count
    out = S.dbscan_lattice(np.array([[0, 0, 0]] + right + left), 4, 4)
    assert out['labels'].tolist() == [0] * 5 + [1] * 4 and not out['core'][0]
    out = S.dbscan_lattice(np.array([[100, 0, 0]] + left + right), 4, 4)
    assert out['labels'].tolist() == [-1] + [0] * 4 + [1] * 4


def test_min_points_one_makes_every_point_core():
    k = np.array([[0, 0, 0], [1, 0, 0], [50, 0, 0], [0, 0, 0]])
    out = S.dbscan_lattice(k, 1, 1)
    assert out['core'].all() and out['labels'].tolist() == [0, 0, 1, 0] and out['sizes'].tolist() == [3, 1] and out['border'].sum() == 0


def test_relabelling_and_centroids():
    labels, core = np.array([2, 2, -1, 0, 1, 0]), np.array([False, True, False, True, True, True])
    assert S.relabel_by_first_core(labels, core).tolist() == [-1, 0, -1, 1, 2, 1]
    x = np.arange(18, dtype=np.float64).reshape(6, 3)
    c = S.centroids(x, labels, 3)
    assert np.array_equal(c[0], (x[3] + x[5]) / 2) and np.array_equal(c[2], (x[0] + x[1]) / 2)


# ---- the conditions the GPU tests rely on -------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _lattice():
    return S.lattice_cloud()


def test_lattice_cloud_is_exact_in_fp32():
    k = _lattice()
    assert 4000 < len(k) < 4800 and np.abs(k).max() <= 500
    x = S.lattice_xyz(k)
    assert np.array_equal(x.astype(np.float64), k * S.UNIT)
    assert len(np.unique(k, axis=0)) <= len(k) - 50                                  # the duplicates are there
    # every squared distance the kernel can meet inside the 27 cells (|d| <= 2 cells of 1.02 r per axis, r <= 50 units) is an integer
    # below 2^24 in units of 2^-20: differences, squares and their sum are exact in fp32, and so is r^2
    assert 3 * (2 * 1.02 * 50 + 1) ** 2 < 2 ** 24


@pytest.mark.parametrize('r,min_points', S.LATTICE_CASES)
def test_lattice_cases_have_pairs_at_the_radius_and_border_points(r, min_points):
    out = S.dbscan_lattice(_lattice(), r, min_points)
    print('r=%d min_points=%d: %d clusters, %d border points, %d pairs exactly at the radius, %d noise' % (
        r, min_points, out['n_clusters'], out['border'].sum(), out['at_radius'], (out['labels'] < 0).sum()))
    assert out['at_radius'] >= 1 and out['n_clusters'] >= 3
    if min_points > 1:                                      # (with min_points = 1 every point is core: there is no border)
        assert out['border'].sum() >= 1
    else:
        assert out['core'].all()
    assert np.float32(r * S.UNIT) == r * S.UNIT             # eps is an fp32 number


@pytest.mark.parametrize('eps,min_points', [(0.01, 4), (0.05, 10)])
def test_real_cloud_labels_do_not_depend_on_the_band_round_eps(eps, min_points):
    import cloud_ref
    x = cloud_ref.cloud_a()[0]
    lo, hi = S.dbscan_real(x, eps * (1 - 1e-5), min_points), S.dbscan_real(x, eps * (1 + 1e-5), min_points)
    print('eps=%g: %d clusters, %d pairs in the band' % (eps, lo['n_clusters'], S.pairs_in_band(x, eps)))
    assert np.array_equal(lo['labels'], hi['labels']) and np.array_equal(lo['core'], hi['core'])
    assert lo['n_clusters'] >= 1 and (lo['labels'] < 0).any()


@pytest.mark.parametrize('h,seed', [(64, 0), (256, 1), (1000, 0)])
def test_plane_scene_conditions(h, seed):
    xyz, on_plane = S.plane_scene()
    out = S.segment_plane(xyz, S.THRESHOLD, h, seed)
    n = out['plane'][:3]
    angle = np.degrees(np.arccos(min(1.0, abs(float(n @ S.PLANE_NORMAL)))))
    inl = np.zeros(len(xyz), bool)
    inl[out['inliers']] = True
    recall, precision = (inl & on_plane).sum() / on_plane.sum(), (inl & on_plane).sum() / inl.sum()
    val = out['eigenvalues']
    print('H=%d seed=%d: best iteration %d with %d inliers, margin %.3g, angle %.4f deg, recall %.4f, precision %.4f, eigenvalues %s' % (
        h, seed, out['best'], out['counts'][out['best']], out['margin'], angle, recall, precision, val))
    assert out['margin'] > 1e-9                              # no point within 1e-9 of the threshold: the inlier set is decided
    assert angle < 0.05 and recall > 0.99 and precision > 0.99
    assert abs(np.linalg.norm(n) - 1.0) < 1e-14 and n[2] > 0
    assert val[1] - val[0] > 0.08                            # the gap that makes the normal well conditioned
    assert (out['counts'] == out['counts'].max()).sum() >= 1 and out['best'] == int(np.argmax(out['counts']))


# ---- the host side of nksr_amd/segment.py --------------------------------------------------------------------------------------------------
def test_module_surface():
    import nksr
    from nksr_amd import build, cloud, segment
    assert 'segment.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'uf_dev.h'))
    for name in ('cluster_dbscan', 'segment_plane', 'plane_scores', 'sample_planes', 'DbscanResult'):
        assert getattr(cloud, name) is getattr(segment, name)
    assert callable(cloud.CloudIndex.cluster_dbscan)
    assert callable(nksr.get_dbscan_preprocess_fn(0.1, 4, keep_largest=1)) and callable(nksr.get_remove_plane_preprocess_fn(0.01))
    assert 'per chunk' in nksr.get_dbscan_preprocess_fn.__doc__
    assert segment.FIELDS * 8 == 256 and segment.P_MOMENT + 6 <= segment.FIELDS


def test_planes_of_triples_and_refinement_match_the_restatement():
    from nksr_amd import segment
    xyz, _ = S.plane_scene()
    x = xyz.astype(np.float64)
    tri = np.random.RandomState(0).randint(0, len(x), (64, 3))
    tri[5] = [7, 7, 9]                                      # a repeated point and three collinear ones: degenerate
    p = x[tri]
    p[9] = [[0, 0, 0], [1, 1, 1], [3, 3, 3]]
    planes = segment.planes_of_triples(p)
    assert np.array_equal(planes[5], np.zeros(4)) and np.array_equal(planes[9], np.zeros(4))
    want, _ = S.sample_planes(xyz, 64, 0)
    ok = np.ones(64, bool)
    ok[[5, 9]] = False
    assert np.array_equal(planes[ok], want[ok])
    # the refinement from packed sums about a centre equals the one from the points about their mean
    out = S.segment_plane(xyz, S.THRESHOLD, 64, 0)
    mask = np.abs(S.residuals(xyz, out['planes'][out['best']])) <= S.THRESHOLD
    centre = 0.5 * (x.min(0) + x.max(0))
    q = x[mask] - centre
    sums = np.zeros(segment.FIELDS)
    sums[segment.P_COUNT] = mask.sum()
    sums[segment.P_SUM:segment.P_SUM + 3] = q.sum(0)
    sums[segment.P_MOMENT:segment.P_MOMENT + 6] = (q.T @ q)[np.triu_indices(3)]
    got = segment.plane_from_moments(sums, centre)
    print('refinement from sums against the restatement: %.3g' % np.abs(got - out['plane']).max())
    assert np.abs(got - out['plane']).max() < 1e-12
    assert segment.plane_from_moments(np.zeros(segment.FIELDS), centre) is None
    for pl, want in (([0, 0, -1, 2], [0, 0, 1, -2]), ([1, -1, 0, 0], [-1, 1, 0, 0]), ([-1, 0, 0, 3], [1, 0, 0, -3]), ([0, 1, 1, 0], [0, 1, 1, 0])):
        assert segment.sign_normal(np.array(pl, float)).tolist() == [float(v) for v in want]
        assert S.sign_normal(np.array(pl, float)).tolist() == [float(v) for v in want]


def test_argument_checks_that_need_no_gpu():
    import torch
    from nksr_amd import segment
    x = torch.zeros((8, 3))
    with pytest.raises(RuntimeError):
        segment.cluster_dbscan(x, 0.1, 4)                   # CPU tensors: the product path is GPU-only
    with pytest.raises(RuntimeError):
        segment.segment_plane(x, 0.01)
    with pytest.raises(RuntimeError):
        segment.plane_scores(x, np.zeros((2, 4)), 0.01)
    with pytest.raises(ValueError):
        segment.segment_plane(x, 0.01, ransac_n=4)
    for eps, m in ((0.0, 4), (-1.0, 4), (float('inf'), 4), (float('nan'), 4), (0.1, 0)):
        with pytest.raises(ValueError):
            segment.cluster_dbscan(x, eps, m)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------------
def test_segment_c_abi_argument_errors_without_a_gpu():
    """Every entry point validates before any launch: error code + message on a machine without a GPU, never an abort.  The pointers
    are host buffers that are never dereferenced (every call ends at a check)."""
    from nksr_amd import _lib
    lib = _lib.lib
    null = C.c_void_p(0)
    buf = (C.c_double * 64)()
    at = C.cast(buf, C.c_void_p)
    nan, inf = float('nan'), float('inf')

    def err():
        return lib.nksr_last_error().decode()

    def comp(n=10, grid=at, hcap=8, cell=0.1, inv_cell=10.0, radius=0.05, core=at, parent=at, flags=at):
        return lib.nksr_dbscan_components(grid, n, grid, grid, grid, grid, hcap, cell, inv_cell, radius, core, parent, flags, null)

    def border(n=10, grid=at, hcap=8, cell=0.1, inv_cell=10.0, radius=0.05, core=at, label=at):
        return lib.nksr_dbscan_border(grid, n, grid, grid, grid, grid, hcap, cell, inv_cell, radius, core, label, null)

    for fn in (comp, border):
        assert fn(n=-1) == _lib.ERR_ARG and '2^31' in err()
        assert fn(n=1 << 31) == _lib.ERR_ARG and '2^31' in err()
        for r in (0.0, -1.0, inf, nan):
            assert fn(radius=r) == _lib.ERR_ARG and 'radius' in err()
        assert fn(grid=null) == _lib.ERR_ARG and 'NULL grid' in err()
        assert fn(hcap=12) == _lib.ERR_ARG and 'power of two' in err()
        assert fn(cell=0.04) == _lib.ERR_ARG and 'must be >= radius' in err()         # cell < radius
        assert fn(cell=nan) == _lib.ERR_ARG
        assert fn(core=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert comp(parent=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert comp(flags=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert comp(n=0, flags=null) == _lib.ERR_ARG and 'NULL arrays' in err()          # (the closing flag is written even for n = 0)
    assert border(label=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert border(n=0, grid=null, core=null, label=null) == 0                        # nothing to do: OK, nothing touched

    assert lib.nksr_dbscan_min_caller(at, at, -1, at, null) == _lib.ERR_ARG and '2^31' in err()
    for k in range(3):
        args = [at, at, 10, at, null]
        args[k if k < 2 else 3] = null
        assert lib.nksr_dbscan_min_caller(*args) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert lib.nksr_dbscan_min_caller(null, null, 0, null, null) == 0

    def score(xyz=at, n=10, planes=at, h=4, t=0.01, counts=at):
        return lib.nksr_plane_score(xyz, n, planes, h, t, counts, null)

    def moments(xyz=at, n=10, plane=at, centre=at, t=0.01, mask=at, partials=at):
        return lib.nksr_plane_moments(xyz, n, plane, centre, t, mask, partials, null)

    for fn in (score, moments):
        assert fn(n=-1) == _lib.ERR_ARG and '2^31' in err()
        for t in (-1e-3, inf, nan):
            assert fn(t=t) == _lib.ERR_ARG and 'threshold' in err()
        assert fn(xyz=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert score(h=-1) == _lib.ERR_ARG and 'n_planes' in err()
    assert score(h=(1 << 20) + 1) == _lib.ERR_ARG and 'n_planes' in err()
    assert score(planes=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert score(counts=null) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert score(h=0, planes=null, counts=null) == 0
    for name in ('plane', 'centre', 'mask', 'partials'):
        assert moments(**{name: null}) == _lib.ERR_ARG and 'NULL arrays' in err()
    assert moments(n=0, xyz=null, plane=null, centre=null, mask=null, partials=null) == 0
