"""nksr_amd/segment.py on the GPU (csrc/segment.hip: k_dbscan_hook, k_dbscan_min_caller, k_dbscan_border, k_hypothesis_score,
k_plane_moments) against tests/segment_ref.py.

Every integer result is compared index for index, nothing is left out.  Where a real-valued input could put a pair or a point on the
wrong side of a threshold by rounding alone, the test asserts a CONDITION on the input (no label changes inside a band round eps; no
point within 1e-9 of the distance threshold) -- tests/test_segment_cpu.py asserts the same conditions without a GPU -- and then asks
for equality.  Tolerances: a centroid is an fp64 mean rounded once to fp32, the reference an fp64 mean in another order: one fp32 ulp.
The refined plane: fp64 sums of ~12 k terms are good to ~1e-12 relative and the eigenvalue gap is 0.083 of the same scale, so the two
planes agree to a few 1e-12; 1e-10 leaves about fifty times that."""
import functools

import numpy as np
import pytest
import torch

import segment_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_dbscan(r, ref, xyz=None):
    labels, core, sizes = r.labels.cpu().numpy(), r.core.cpu().numpy(), r.sizes.cpu().numpy()
    assert labels.dtype == np.int64 and core.dtype == np.bool_ and sizes.dtype == np.int64 and isinstance(r.n_clusters, int)
    assert np.array_equal(core, ref['core'])
    assert r.n_clusters == ref['n_clusters']
    assert np.array_equal(labels, ref['labels'])
    assert np.array_equal(sizes, ref['sizes'])
    assert tuple(r.centroid.shape) == (r.n_clusters, 3) and r.centroid.dtype == torch.float32
    if xyz is not None and r.n_clusters:
        want = S.centroids(xyz, ref['labels'], ref['n_clusters'])
        got = r.centroid.cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print('centroids: max error %.3g ulp' % (np.abs(got - want) / ulp).max())
        assert (np.abs(got - want) <= ulp).all()


# ---- 1. exact on a lattice cloud -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _lattice():
    k = S.lattice_cloud()
    return k, S.lattice_xyz(k)


@functools.lru_cache(None)
def _lattice_index():
    from nksr_amd import cloud
    return cloud.CloudIndex(_gpu(_lattice()[1]))


@pytest.mark.parametrize('r,min_points', S.LATTICE_CASES)
def test_dbscan_exact_on_the_lattice_cloud(r, min_points):
    k, x = _lattice()
    ref = S.dbscan_lattice(k, r, min_points)
    assert ref['at_radius'] >= 1 and (min_points == 1 or ref['border'].sum() >= 1)
    got = _lattice_index().cluster_dbscan(r * S.UNIT, min_points)
    print('r=%d min_points=%d: %d clusters, %d border points, %d pairs at the radius' % (r, min_points, ref['n_clusters'], ref['border'].sum(),
                                                                                       ref['at_radius']))
    _check_dbscan(got, ref, x)


# ---- 2. a real-valued cloud ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps,min_points', [(0.01, 4), (0.05, 10)])
def test_dbscan_on_a_real_valued_cloud(eps, min_points):
    import cloud_ref
    from nksr_amd import cloud
    x = cloud_ref.cloud_a()[0]
    lo, hi = S.dbscan_real(x, eps * (1 - 1e-5), min_points), S.dbscan_real(x, eps * (1 + 1e-5), min_points)
    # the condition on the input: no label and no core flag depends on the pairs inside the band round eps
    assert np.array_equal(lo['labels'], hi['labels']) and np.array_equal(lo['core'], hi['core'])
    _check_dbscan(cloud.cluster_dbscan(_gpu(x), eps, min_points), lo, x)


# ---- 3. shapes where the kernels can go wrong -------------------------------------------------------------------------------------------------
def _run_lattice(k, r, min_points):
    from nksr_amd import cloud
    k = np.asarray(k, np.int64).reshape(-1, 3)
    x = S.lattice_xyz(k)
    got = cloud.cluster_dbscan(_gpu(x), r * S.UNIT, min_points)
    ref = S.dbscan_lattice(k, r, min_points)
    _check_dbscan(got, ref, x)
    return ref


def test_dbscan_single_point():
    assert _run_lattice([[7, -3, 2]], 5, 1)['labels'].tolist() == [0]
    assert _run_lattice([[7, -3, 2]], 5, 2)['labels'].tolist() == [-1]


@pytest.mark.parametrize('n', [127, 128, 129, 300])
def test_dbscan_copies_of_one_point(n):
    """a whole block of lanes (and one more, one less) in one cell: the scan's groups of four and its tail; min_points = N is reached
    by the point itself and its N - 1 copies, N + 1 by nothing"""
    k = np.tile([[11, 12, -13]], (n, 1))
    ref = _run_lattice(k, 3, n)
    assert ref['n_clusters'] == 1 and ref['sizes'].tolist() == [n]
    ref = _run_lattice(k, 3, n + 1)
    assert ref['n_clusters'] == 0 and (ref['labels'] == -1).all()


def test_dbscan_two_points_exactly_eps_apart():
    assert _run_lattice([[0, 0, 0], [3, 4, 0]], 5, 2)['labels'].tolist() == [0, 0]
    assert _run_lattice([[0, 0, 0], [3, 4, 0]], 4, 2)['labels'].tolist() == [-1, -1]
    assert _run_lattice([[100, 200, -300], [100 + 12, 200 - 4, -300 + 3]], 13, 2)['labels'].tolist() == [0, 0]


def test_dbscan_everything_noise():
    k = _lattice()[0]
    k = np.unique(k, axis=0)                                # no duplicates: at r < 1 nothing has a neighbour
    k = k[np.random.RandomState(0).permutation(len(k))]
    ref = _run_lattice(k, 0.5, 2)
    assert ref['n_clusters'] == 0 and (ref['labels'] == -1).all() and not ref['core'].any()


def test_dbscan_long_chain_is_one_cluster():
    """2 000 points spaced exactly eps along x, shuffled: one cluster across many workgroups -- every hook but the first meets a tree
    that other lanes are changing (retries), and the flatten pass has long paths to walk"""
    n = 2000
    k = np.stack([np.arange(n) - n // 2, np.full(n, 3), np.full(n, -7)], axis=1)
    k = k[np.random.RandomState(4).permutation(n)]
    ref = _run_lattice(k, 1, 2)
    assert ref['n_clusters'] == 1 and ref['core'].all() and ref['at_radius'] == n - 1
    ref = _run_lattice(k, 1, 3)                             # the two ends become border points
    assert ref['n_clusters'] == 1 and ref['border'].sum() == 2


def test_dbscan_empty_cloud_and_errors():
    from nksr_amd import cloud
    got = cloud.cluster_dbscan(torch.zeros((0, 3), device=DEV), 0.1, 4)
    assert got.n_clusters == 0 and got.labels.shape == (0,) and got.labels.dtype == torch.int64 and got.core.dtype == torch.bool
    assert got.sizes.shape == (0,) and tuple(got.centroid.shape) == (0, 3) and got.labels.device.type == 'cuda'
    x = _gpu(_lattice()[1])
    for eps, m in ((0.0, 4), (float('nan'), 4), (0.1, 0)):
        with pytest.raises(ValueError):
            cloud.cluster_dbscan(x, eps, m)
    with pytest.raises(RuntimeError):
        cloud.cluster_dbscan(x.cpu(), 0.1, 4)
    bad = x.clone()
    bad[5, 1] = float('nan')
    with pytest.raises(RuntimeError):
        cloud.cluster_dbscan(bad, 0.1, 4)


# ---- 4. repeatability and the permutation rule -----------------------------------------------------------------------------------------------
def test_dbscan_repeats_bit_for_bit_and_follows_the_caller_order():
    from nksr_amd import cloud
    k, x = _lattice()
    r, m = 13, 6
    a = cloud.cluster_dbscan(_gpu(x), r * S.UNIT, m)
    b = cloud.cluster_dbscan(_gpu(x), r * S.UNIT, m)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.sizes, b.sizes) and torch.equal(a.core, b.core)
    assert torch.equal(a.centroid.view(torch.int32), b.centroid.view(torch.int32))
    # a shuffled caller order: the same core points; their clusters are the same sets, numbered by the new order (a border point
    # between two clusters may change sides with the numbering, so all labels are compared with the restatement of the shuffled cloud)
    p = np.random.RandomState(9).permutation(len(k))
    c = cloud.cluster_dbscan(_gpu(x[p]), r * S.UNIT, m)
    la, ca, lc, cc = a.labels.cpu().numpy(), a.core.cpu().numpy(), c.labels.cpu().numpy(), c.core.cpu().numpy()
    assert np.array_equal(cc, ca[p])
    assert np.array_equal(np.where(cc, lc, -1), S.relabel_by_first_core(la[p], ca[p]))
    _check_dbscan(c, S.dbscan_lattice(k[p], r, m), x[p])


# ---- 5. plane scores --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _scene():
    return S.plane_scene()


@pytest.mark.parametrize('h', [64, 256, 1000])
def test_plane_scores_exact(h):
    from nksr_amd import cloud
    xyz = _scene()[0]
    planes, triples = cloud.sample_planes(_gpu(xyz), h, seed=0)
    want_planes, bad = S.sample_planes(xyz, h, 0)
    assert planes.dtype == np.float64 and np.array_equal(planes, want_planes)
    assert np.array_equal(triples, np.random.RandomState(0).randint(0, len(xyz), (h, 3)))
    # degenerate hypotheses among the others: zero rows (what a collinear triple gives) and a row that is not finite
    planes = planes.copy()
    planes[[3, h // 2, h - 1]] = 0.0
    planes[7, 1] = np.nan
    want = S.plane_counts(xyz, planes, S.THRESHOLD)
    assert (want[[3, 7, h // 2, h - 1]] == -1).all() and (want >= 0).sum() == h - 4
    got = cloud.plane_scores(_gpu(xyz), planes, S.THRESHOLD)
    assert got.dtype == torch.int32 and got.device.type == 'cuda'
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, cloud.plane_scores(_gpu(xyz), torch.from_numpy(planes), S.THRESHOLD))


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1023, 1025])
def test_plane_scores_count_every_point_of_a_small_cloud(n):
    """one workgroup's last lanes, and one point more than a workgroup holds: all of them must be counted"""
    from nksr_amd import cloud
    rs = np.random.RandomState(n)
    xyz = np.concatenate([rs.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], axis=1).astype(np.float32)          # on z = 0
    xyz[:, 2] = (rs.randint(-2, 3, n) * 2.0 ** -12).astype(np.float32)
    planes = np.concatenate([cloud.sample_planes(_gpu(xyz), 8, seed=1)[0], [[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 2.0 ** -12], [0.0, 0.0, 0.0, 0.0]]])
    for t in (2.0 ** -11, 2.0 ** -12, 0.0):                 # (exact numbers: a point AT the threshold counts)
        want = S.plane_counts(xyz, planes, t)
        got = cloud.plane_scores(_gpu(xyz), planes, t).cpu().numpy()
        assert np.array_equal(got, want)
        assert want[-1] == -1 and (t < 2.0 ** -11 or want[-3] == n)


@pytest.mark.parametrize('h', [1, 127, 128, 129])
@pytest.mark.parametrize('n', [0, 1, 1023, 1024, 1025])
def test_plane_scores_at_the_edges_of_the_scorer(n, h):
    """No point, one, and one less / exactly / one more than the 4 x 256 a workgroup holds, against one plane, one less / exactly / one
    more than the 128 a workgroup stages: exact counts.  A degenerate plane first, last and -- h = 129 -- alone in the last chunk: -1."""
    from nksr_amd import cloud
    rs = np.random.RandomState(1000 * h + n)
    xyz = rs.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    normal = rs.normal(size=(h, 3))
    planes = np.concatenate([normal / np.linalg.norm(normal, axis=1, keepdims=True), rs.uniform(-0.3, 0.3, (h, 1))], axis=1)
    bad = sorted({0, h - 1})
    planes[bad] = 0.0
    t = 0.1
    good = np.setdiff1d(np.arange(h), bad)
    gap = min([np.abs(np.abs(S.residuals(xyz, planes[k])) - t).min() for k in good if n], default=1.0)
    assert gap > 1e-9                                       # no count hangs on the last bits of a residual
    want = S.plane_counts(xyz, planes, t)
    got = cloud.plane_scores(_gpu(xyz), planes, t).cpu().numpy()
    assert np.array_equal(got, want)
    assert (want[bad] == -1).all() and (want[good] >= 0).all() and (n < 1023 or h < 127 or want.max() > 0)


# ---- 6. segment_plane end to end----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,seed', [(64, 0), (256, 1), (1000, 0)])
def test_segment_plane_end_to_end(h, seed):
    from nksr_amd import cloud
    xyz, on_plane = _scene()
    ref = S.segment_plane(xyz, S.THRESHOLD, h, seed)
    assert ref['margin'] > 1e-9                              # the condition on the input: no point within 1e-9 of the threshold
    xg = _gpu(xyz)
    counts = cloud.plane_scores(xg, cloud.sample_planes(xg, h, seed)[0], S.THRESHOLD).cpu().numpy()
    assert np.array_equal(counts, ref['counts']) and int(np.argmax(counts)) == ref['best']
    plane, inliers = cloud.segment_plane(xg, S.THRESHOLD, num_iterations=h, seed=seed)
    assert isinstance(plane, np.ndarray) and plane.dtype == np.float64 and plane.shape == (4,)
    assert inliers.dtype == torch.int64 and inliers.device.type == 'cuda'
    print('H=%d seed=%d: best %d; plane against the restatement: %.3g' % (h, seed, ref['best'], np.abs(plane - ref['plane']).max()))
    assert abs(np.linalg.norm(plane[:3]) - 1.0) < 1e-14
    assert np.abs(plane - ref['plane']).max() < 1e-10
    assert np.array_equal(inliers.cpu().numpy(), ref['inliers'])
    # against the analytic plane
    angle = np.degrees(np.arccos(min(1.0, abs(float(plane[:3] @ S.PLANE_NORMAL)))))
    inl = np.zeros(len(xyz), bool)
    inl[inliers.cpu().numpy()] = True
    recall, precision = (inl & on_plane).sum() / on_plane.sum(), (inl & on_plane).sum() / inl.sum()
    print('angle %.4f deg, recall %.4f, precision %.4f' % (angle, recall, precision))
    assert angle < 0.05 and recall > 0.99 and precision > 0.99
    # the same call gives the same bits
    plane2, inliers2 = cloud.segment_plane(xg, S.THRESHOLD, num_iterations=h, seed=seed)
    assert np.array_equal(plane, plane2) and torch.equal(inliers, inliers2)


def test_segment_plane_errors():
    from nksr_amd import cloud
    xg = _gpu(_scene()[0])
    with pytest.raises(ValueError):
        cloud.segment_plane(xg, S.THRESHOLD, ransac_n=4)
    with pytest.raises(ValueError):
        cloud.segment_plane(xg, -1.0)
    with pytest.raises(ValueError):
        cloud.segment_plane(xg[:2], S.THRESHOLD)
    with pytest.raises(RuntimeError):                        # one point, many times: every triple is degenerate
        cloud.segment_plane(xg[:1].repeat(50, 1), S.THRESHOLD, num_iterations=16)


# ---- 7. preprocess makers -----------------------------------------------------------------------------------------------------------------------
def test_preprocess_makers_equal_the_steps_by_hand():
    import nksr
    xyz = _scene()[0]
    xg = _gpu(xyz)
    ng, sg = xg * 2.0, xg + 1.0
    fn = nksr.compose_preprocess_fns(nksr.get_remove_plane_preprocess_fn(S.THRESHOLD, num_iterations=256, seed=1),
                                     nksr.get_dbscan_preprocess_fn(0.02, 6, keep_largest=1))
    x2, n2, s2 = fn(xg, ng, sg)
    _, inliers = nksr.cloud.segment_plane(xg, S.THRESHOLD, num_iterations=256, seed=1)
    keep = torch.ones(len(xyz), dtype=torch.bool, device=DEV)
    keep[inliers] = False
    rest = xg[keep]
    r = nksr.cloud.cluster_dbscan(rest, 0.02, 6)
    largest = int(torch.argmax(r.sizes))                     # (the first of the maxima: the lower label on a tie)
    assert r.n_clusters >= 4 and int(r.sizes[largest]) >= 400         # (eight spheres, some of them touching)
    pick = r.labels == largest
    assert torch.equal(x2, rest[pick]) and torch.equal(n2, ng[keep][pick]) and torch.equal(s2, sg[keep][pick])
    # min_cluster_size, both together, and None passing through
    x3, n3, s3 = nksr.get_dbscan_preprocess_fn(0.02, 6, min_cluster_size=100)(rest, None, None)
    big = (r.sizes >= 100)[r.labels.clamp(min=0)] & (r.labels >= 0)
    assert n3 is None and s3 is None and torch.equal(x3, rest[big]) and 0 < x3.shape[0] < rest.shape[0]
    x4, _, _ = nksr.get_dbscan_preprocess_fn(0.02, 6, min_cluster_size=100, keep_largest=2)(rest, None, None)
    top2 = torch.sort(r.sizes, descending=True, stable=True)[1][:2]
    assert torch.equal(x4, rest[(r.labels == top2[0]) | (r.labels == top2[1])])


def test_composed_preprocess_fn_in_front_of_reconstruct():
    import nksr
    from nksr_amd import utils
    sphere, sn = utils.synth_sphere(6000, 0.25, 0.001, 0)
    rs = np.random.RandomState(3)
    gxy = rs.uniform(-0.5, 0.5, (6000, 2))
    ground = np.concatenate([gxy, np.full((6000, 1), -0.4)], axis=1).astype(np.float32)
    gn = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (6000, 1))
    xg, ng = _gpu(np.concatenate([sphere, ground])), _gpu(np.concatenate([sn, gn]))
    fn = nksr.compose_preprocess_fns(nksr.get_remove_plane_preprocess_fn(0.005, num_iterations=64), nksr.get_dbscan_preprocess_fn(0.03, 6, keep_largest=1))
    x2, n2, _ = fn(xg, ng, None)
    assert torch.equal(x2, xg[:6000]) and torch.equal(n2, ng[:6000])          # the ground is gone, the sphere is whole and in order
    field = nksr.Reconstructor(torch.device(DEV)).reconstruct(xg, ng, preprocess_fn=fn, voxel_size=0.05)
    mesh = field.extract_dual_mesh(mise_iter=1)
    assert mesh.v.shape[0] > 100 and float(mesh.v[:, 2].min()) > -0.35        # the surface of the sphere alone
