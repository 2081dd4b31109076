"""nksr_amd/orient.py on the GPU (csrc/orient.hip) against tests/orient_ref.py: Kruskal in numpy on the SAME neighbour table, compared
for exact equality -- every edge key is a distinct integer, so the minimum spanning forest, the signs and the labels are unique and
no tolerance enters.  Analytic shapes: every output normal must agree with the true one (100 %: the CPU reference does so on these
inputs, with one component each)."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref
import orient_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VIEWPOINT = (0.1, -0.2, 2.0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _random_flips(nrm, seed=3):
    sign = np.where(np.random.RandomState(seed).rand(len(nrm)) < 0.5, -1.0, 1.0).astype(np.float32)
    return (nrm * sign[:, None]).astype(np.float32)


def _check_exact(xyz, normal, idx, viewpoint=None, order=None, stats=None):
    """orient_graph == the reference, bit for bit; -> the GPU result"""
    from nksr_amd import cloud
    res = cloud.orient_graph(_gpu(xyz), _gpu(normal), idx if torch.is_tensor(idx) else _gpu(idx), viewpoint=viewpoint, order=order, stats=stats)
    flipped, comp, ncomp = R.orient(xyz, normal, _np(idx) if torch.is_tensor(idx) else idx, viewpoint=viewpoint)
    assert res.flipped.dtype == torch.uint8 and res.component.dtype == torch.int32 and res.normal.dtype == torch.float32
    assert res.n_components == ncomp
    assert np.array_equal(_np(res.component), comp)
    assert np.array_equal(_np(res.flipped), flipped)
    assert np.array_equal(_np(res.normal).view(np.uint32), R.apply(normal, flipped).view(np.uint32))
    return res


# ---- 1. exact equality on real neighbour tables --------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _input(name):
    """(xyz, unoriented normals) in the caller's order"""
    if name == 'cloud_a':
        xyz, nrm = cloud_ref.cloud_a()
        return xyz, _random_flips(nrm)
    import os
    from nksr_amd import normals
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bunny_2k.npz'))
    xyz = d['xyz'].astype(np.float32)
    pg, nrm, _, valid = normals.knn_pca(_gpu(xyz), 16)              # the bunny's PCA normals: unoriented, zero where the kernel found none
    out = torch.zeros_like(nrm)
    out[pg.perm] = torch.where((valid > 0)[:, None], nrm, torch.zeros_like(nrm))
    return xyz, _np(out)


@functools.lru_cache(None)
def _table(name, k):
    from nksr_amd import cloud
    index = cloud.CloudIndex(_gpu(_input(name)[0]))
    idx, _ = index.knn(k, exclude_self=True)
    return index, idx


@pytest.mark.parametrize('viewpoint', [None, VIEWPOINT], ids=['+z', 'viewpoint'])
@pytest.mark.parametrize('name,k', [('bunny_2k', 8), ('bunny_2k', 16), ('cloud_a', 8)])
def test_matches_reference_exactly(name, k, viewpoint):
    xyz, nrm = _input(name)
    index, idx = _table(name, k)
    res = _check_exact(xyz, nrm, idx, viewpoint)
    print('%s k=%d: %d components, %.3f flipped' % (name, k, res.n_components, float(res.flipped.float().mean())))
    # the same through the index (the kernels then visit the points in Morton order: nothing may change), and through orient_normals
    via = index.orient_normals(_gpu(nrm), k=k, viewpoint=viewpoint)
    assert via.n_components == res.n_components
    for a, b in zip(via[:3], res[:3]):
        assert torch.equal(a, b)
    if name == 'bunny_2k':
        from nksr_amd import cloud
        top = cloud.orient_normals(_gpu(xyz), _gpu(nrm), k=k, viewpoint=viewpoint)
        assert top.n_components == res.n_components and all(torch.equal(a, b) for a, b in zip(top[:3], res[:3]))


# ---- 2. analytic shapes ------------------------------------------------------------------------------------------------------------
def _shape(kind, noise):
    from nksr_amd import utils
    if kind == 'sphere':
        return utils.synth_sphere(2000, 0.45, noise)
    if kind == 'torus':
        return utils.synth_torus(3000, 0.32, 0.12, noise)
    return utils.synth_rounded_box(3000)


@pytest.mark.parametrize('k', [8, 16])
@pytest.mark.parametrize('kind,noise', [('sphere', 0.0), ('sphere', 0.005), ('torus', 0.0), ('torus', 0.005), ('rbox', 0.0)])
def test_analytic_shapes_come_out_oriented(kind, noise, k):
    from nksr_amd import cloud
    xyz, nrm = _shape(kind, noise)
    xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
    given = _random_flips(nrm)
    res = cloud.orient_normals(_gpu(xyz), _gpu(given), k=k)
    agree = float(((_np(res.normal) * nrm).sum(1) > 0).mean())
    print('%s noise %g k=%d: agreement %.4f, components %d' % (kind, noise, k, agree, res.n_components))
    assert res.n_components == 1
    assert agree == 1.0
    assert np.array_equal(_np(res.normal), np.where(_np(res.flipped)[:, None] != 0, -given, given))


# ---- 3. two spheres ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [8, 16])
def test_two_spheres_are_signed_separately(k):
    from nksr_amd import cloud, utils
    a, na = utils.synth_sphere(1500, 0.2, 0.0, 0, center=(-0.3, 0.0, 0.0))
    b, nb = utils.synth_sphere(1500, 0.2, 0.0, 1, center=(0.3, 0.0, 0.0))
    xyz, nrm = np.concatenate([a, b]).astype(np.float32), np.concatenate([na, nb]).astype(np.float32)
    given = _random_flips(nrm)
    res = cloud.orient_normals(_gpu(xyz), _gpu(given), k=k)
    assert res.n_components == 2
    comp = _np(res.component)
    assert (comp[:1500] == 0).all() and (comp[1500:] == 1).all()
    assert ((_np(res.normal) * nrm).sum(1) > 0).all()
    # the viewpoint at the centre of the first sphere: that sphere looks at it (inward), the other one too (its near side faces it)
    res = cloud.orient_normals(_gpu(xyz), _gpu(given), k=k, viewpoint=(-0.3, 0.0, 0.0))
    out = (_np(res.normal) * nrm).sum(1)
    assert res.n_components == 2 and (out[:1500] < 0).all() and (out[1500:] > 0).all()


# ---- 4. explicit small graphs ----------------------------------------------------------------------------------------------------------
def _points(n, seed=0):
    rs = np.random.RandomState(seed)
    nrm = rs.randn(n, 3)
    return rs.uniform(-1, 1, (n, 3)).astype(np.float32), (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)


def test_path_with_decreasing_weights_is_one_long_chain():
    """4096 nodes i -> i + 1 whose weights strictly decrease: in round 1 every node links to its successor, one chain of 4095 links
    that the pointer doubling must flatten."""
    n = 4096
    theta = np.linspace(1.2, 0.2, n - 1)                            # angle between consecutive normals: w = 1 - cos(theta)
    phi = np.concatenate([[0.0], np.cumsum(theta)])
    nrm = _random_flips(np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], 1).astype(np.float32))
    xyz = _points(n)[0]
    idx = np.arange(1, n + 1, dtype=np.int32).reshape(n, 1)
    idx[-1, 0] = -1
    key, _, _, _ = R.edge_keys(nrm, idx)
    assert len(key) == n - 1 and (np.diff((key >> np.uint64(32)).astype(np.int64)) < 0).all()
    stats = {}
    res = _check_exact(xyz, nrm, idx, stats=stats)
    assert res.n_components == 1
    assert stats['rounds'][0]['links'] == n - 1 and len(stats['rounds']) == 1
    _check_exact(xyz, nrm, idx, viewpoint=VIEWPOINT)


def test_grid_of_identical_normals_ties_resolved_by_slot():
    m = 17
    ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing='ij'), -1).reshape(-1, 2)
    idx = np.full((m * m, 4), -1, np.int32)
    for c, (di, dj) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        a, b = ij[:, 0] + di, ij[:, 1] + dj
        ok = (a >= 0) & (a < m) & (b >= 0) & (b < m)
        idx[ok, c] = (a * m + b)[ok]
    nrm = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (m * m, 1))
    xyz = np.concatenate([ij.astype(np.float32), np.zeros((m * m, 1), np.float32)], 1)      # all z equal: the seed is the lowest index
    res = _check_exact(xyz, nrm, idx)
    assert res.n_components == 1 and int(res.flipped.sum()) == 0
    res = _check_exact(xyz, -nrm, idx)
    assert int(res.flipped.sum()) == m * m
    _check_exact(xyz, _random_flips(nrm), idx, viewpoint=(8.0, 8.0, -3.0))


def test_star_whose_hub_lists_nobody():
    n = 40
    xyz, nrm = _points(n, 1)
    idx = np.full((n, 2), -1, np.int32)
    idx[1:, 0] = 0
    res = _check_exact(xyz, nrm, idx)
    assert res.n_components == 1
    _check_exact(xyz, nrm, idx, viewpoint=VIEWPOINT)


def test_rows_with_self_duplicate_negative_and_large_entries():
    n = 50
    xyz, nrm = _points(n, 2)
    idx = np.random.RandomState(5).randint(-3, n + 3, (n, 5)).astype(np.int32)
    idx[::3, 1] = np.arange(n, dtype=np.int32)[::3]                 # self
    idx[::4, 3] = idx[::4, 2]                                       # duplicates
    idx[7] = [-1, n, 7, -2, n + 1]                                  # a row with nothing valid
    _check_exact(xyz, nrm, idx)
    _check_exact(xyz, nrm, _gpu(idx.astype(np.int64)), viewpoint=VIEWPOINT)
    big = idx.astype(np.int64)
    big[big >= n] += 1 << 40                                        # what does not fit int32 is ignored, not wrapped
    res = _check_exact(xyz, nrm, _gpu(big))
    assert np.array_equal(_np(res.flipped), R.orient(xyz, nrm, idx)[0])


@pytest.mark.parametrize('n', [2, 65])
def test_tiny_and_one_more_than_a_wavefront(n):
    xyz, nrm = _points(n, n)
    if n == 2:
        for idx in ([[1], [0]], [[1], [-1]], [[-1], [0]], [[0], [1]]):
            _check_exact(xyz, nrm, np.array(idx, np.int32))
            _check_exact(xyz, nrm, np.array(idx, np.int32), viewpoint=VIEWPOINT)
    else:
        idx = np.stack([(np.arange(n) + 1) % n, (np.arange(n) - 1) % n], 1).astype(np.int32)
        res = _check_exact(xyz, nrm, idx)
        assert res.n_components == 1
        _check_exact(xyz, nrm, idx[:, :1], viewpoint=VIEWPOINT)


def test_isolated_points_and_zero_normals():
    n = 300
    xyz, nrm = _points(n, 4)
    res = _check_exact(xyz, nrm, np.full((n, 3), -1, np.int32))
    assert res.n_components == n and np.array_equal(_np(res.component), np.arange(n))
    assert np.array_equal(_np(res.flipped), (nrm[:, 2] < 0).astype(np.uint8))
    # zero normals in a connected graph: their edges weigh 1 and flip nothing
    nrm[::5] = 0
    idx = np.random.RandomState(6).randint(0, n, (n, 4)).astype(np.int32)
    _check_exact(xyz, nrm, idx)
    _check_exact(xyz, np.zeros_like(nrm), idx, viewpoint=VIEWPOINT)


def test_argument_errors_on_the_gpu():
    from nksr_amd import cloud, normals
    xyz, nrm = _points(20, 7)
    x, nr = _gpu(xyz), _gpu(nrm)
    idx = torch.zeros((20, 2), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='<= 32'):
        cloud.orient_graph(x, nr, torch.zeros((20, 33), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='<= 32'):
        cloud.orient_normals(x, nr, k=0)
    with pytest.raises(ValueError, match='other points'):
        cloud.orient_normals(x, nr, k=20)
    with pytest.raises(ValueError, match='other points'):
        cloud.CloudIndex(x).orient_normals(nr, k=20)
    with pytest.raises(RuntimeError, match='integer'):
        cloud.orient_graph(x, nr, idx.float())
    with pytest.raises(RuntimeError, match='integer'):
        cloud.orient_graph(x, nr, idx[:10])
    with pytest.raises(RuntimeError, match='normal'):
        cloud.orient_graph(x, nr[:10], idx)
    bad = nr.clone()
    bad[3, 1] = float('nan')
    with pytest.raises(RuntimeError, match='finite'):
        cloud.orient_graph(x, bad, idx)
    bad[3, 1] = float('inf')
    with pytest.raises(RuntimeError, match='finite'):
        cloud.orient_normals(x, bad, k=4)
    with pytest.raises(normals.TooFewPoints):
        cloud.estimate_normals(x, knn=64)
    empty = cloud.orient_graph(x[:0], nr[:0], idx[:0])
    assert empty.n_components == 0 and empty.normal.shape == (0, 3) and empty.flipped.shape == (0,) and empty.component.shape == (0,)
    empty = cloud.orient_normals(x[:0], nr[:0], k=4)
    assert empty.n_components == 0 and empty.flipped.dtype == torch.uint8 and empty.component.dtype == torch.int32
    one = cloud.orient_graph(x[:1], -nr[:1].abs(), idx[:1])
    assert one.n_components == 1 and one.flipped.tolist() == [1] and float(one.normal[0, 2]) >= 0


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    xyz, nrm = _input('cloud_a')
    index, idx = _table('cloud_a', 8)
    a = index.orient_normals(_gpu(nrm), k=8)
    b = index.orient_normals(_gpu(nrm), k=8)
    assert a.n_components == b.n_components
    assert torch.equal(a.flipped, b.flipped) and torch.equal(a.component, b.component)
    assert torch.equal(a.normal.view(torch.int32), b.normal.view(torch.int32))


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------
def test_reconstruct_from_positions_only():
    import nksr
    from conftest import make_cloud
    dev = torch.device(DEV)
    xyz, nrm = make_cloud('sphere', 3000)
    x = torch.from_numpy(xyz).to(dev)
    rec = nksr.Reconstructor(dev)
    fld = rec.reconstruct(x, preprocess_fn=nksr.get_estimate_oriented_normal_preprocess_fn(knn=32, orient_k=16), detail_level=None)
    ref = rec.reconstruct(x, torch.from_numpy(nrm).to(dev), detail_level=None)
    centre = torch.zeros((1, 3), device=dev)
    f0, f1 = float(fld.evaluate_f(centre).value[0]), float(ref.evaluate_f(centre).value[0])
    print('field at the centre: %g from estimated normals, %g from the analytic ones' % (f0, f1))
    assert f1 != 0 and np.sign(f0) == np.sign(f1)
    mesh = fld.extract_dual_mesh(mise_iter=1)
    assert mesh.f.shape[0] > 100 and mesh.topology().is_watertight
    # the normals themselves: all outward
    xs, ns = nksr.cloud.estimate_normals(x, knn=32, orient_k=16)
    assert xs.shape[0] > 2900 and bool(((xs * ns).sum(1) > 0).all())
    # the sensor-based function without a sensor raises as before
    with pytest.raises(RuntimeError, match='please provide sensor positions'):
        rec.reconstruct(x, preprocess_fn=nksr.get_estimate_normal_preprocess_fn())
