"""GPU kNN kernels (csrc/knn_normals.hip, knn_query.hip): kNN-PCA normals + sensor orientation (the preprocess_fn of
examples/recons_waymo_cpu.py:21-41) and the nearest-neighbour colour field (PCNNField,
examples/recons_colored_mesh.py:28) against scipy cKDTree / numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _recipe_numpy(xyz, sensor, knn, deg):
    """examples/recons_waymo_cpu.py:21-41 with cKDTree + eigh in place of point_cloud_utils."""
    from scipy.spatial import cKDTree
    _, nb = cKDTree(xyz).query(xyz, k=knn)
    p = xyz[nb].astype(np.float64)
    d = p - p.mean(1, keepdims=True)
    cov = np.einsum('nki,nkj->nij', d, d)
    w, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0].astype(np.float32)
    view = sensor - xyz
    view = view / (np.linalg.norm(view, axis=-1, keepdims=True) + 1e-6)
    cos = (view * nrm).sum(1)
    nrm[cos < 0] *= -1
    keep = np.abs(cos) > np.cos(np.deg2rad(deg))
    return nrm, keep, cos


def test_knn_pca_normals_match_kdtree():
    import nksr
    from nksr_amd import utils
    dev = torch.device('cuda:0')
    xyz, radial = utils.synth_sphere(20000, 1.0, 0.002, seed=5)
    extra, _ = utils.synth_torus(8000, 0.6, 0.2, 0.002, seed=6, center=(3.0, 0.0, 0.0))   # second density
    xyz = np.concatenate([xyz, extra]).astype(np.float32)
    sensor = np.tile(np.array([[8.0, 6.0, 10.0]], np.float32), (len(xyz), 1))
    knn, deg = 32, 85.0
    fn = nksr.get_estimate_normal_preprocess_fn(knn, deg)
    x2, n2, s2 = fn(torch.from_numpy(xyz).to(dev), None, torch.from_numpy(sensor).to(dev))
    assert s2 is None and x2.shape == n2.shape and x2.shape[0] > 0.7 * len(xyz)
    nrm_o, keep_o, cos_o = _recipe_numpy(xyz, sensor, knn, deg)
    # kept set: identical except for points whose |cos| sits at the threshold
    sure = np.abs(np.abs(cos_o) - np.cos(np.deg2rad(deg))) > 0.05   # normals agree to ~2 degrees
    from scipy.spatial import cKDTree
    d, j = cKDTree(xyz).query(x2.cpu().numpy())
    assert d.max() == 0.0                                   # returned points are input points
    kept_gpu = np.zeros(len(xyz), bool)
    kept_gpu[j] = True
    assert (kept_gpu[sure] == keep_o[sure]).all()
    assert (kept_gpu != keep_o).mean() < 0.01
    # order preserved (stable w.r.t. the input order, like boolean masking in the recipe)
    assert (np.diff(j) > 0).all()
    # normals: same direction as the exact-kNN PCA (sign included, after the sensor flip)
    dots = (n2.cpu().numpy() * nrm_o[j]).sum(1)
    assert (dots > 0.999).mean() > 0.995 and dots.min() > 0.9
    np.testing.assert_allclose(np.linalg.norm(n2.cpu().numpy(), axis=1), 1.0, atol=1e-4)
    # and they face the sensor
    view = sensor[j] - x2.cpu().numpy()
    assert ((view * n2.cpu().numpy()).sum(1) > 0).all()


def _normal_clouds(case):
    """(points, cell or None = choose_cell_size, the values `todo` must hold, number of leading sphere points)"""
    from nksr_amd import utils
    sphere, _ = utils.synth_sphere(3000, 1.0, 0.002, seed=5)
    if case == 'wave':
        return sphere, None, {0}, 3000
    if case == 'thread':            # cell 2.5: every 3^3 block holds all 3000 > KW_CAP points, the wavefront kernel hands every query back
        return sphere, 2.5, {1}, 3000
    blob = np.random.RandomState(11).randn(2500, 3) * 0.01 + np.array([3.0, 0.0, 0.0])      # its blocks overflow, the sphere's do not
    return np.concatenate([sphere[:1500], blob]).astype(np.float32), None, {0, 1}, 1500


@pytest.mark.parametrize('case', ['wave', 'thread', 'both'])
def test_thread_per_query_normals_equal_the_wavefront_normals_and_take_what_it_hands_back(case):
    """nksr_knn_pca_normals with a `todo` array (k_knn_pca_wave, then k_knn_pca_normals for the queries it handed back) and without
    (k_knn_pca_normals for every query): the same valid flags and bit-equal k-th distances, and each within the bounds
    test_gpu_pins.py::test_knn_neighbour_sets_equal_the_kdtree_sets holds the default path to against an fp64 kd-tree."""
    from scipy.spatial import cKDTree
    import parity_util as pu
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import PointGrid, _grid_args, choose_cell_size
    dev = torch.device('cuda:0')
    knn = 16
    xyz, cell, todo_values, n_sphere = _normal_clouds(case)
    xt = torch.from_numpy(xyz).to(dev)
    pg = PointGrid(xt, cell if cell else choose_cell_size(xt, knn))
    n = len(xyz)
    x64 = pg.xyz.cpu().numpy().astype(np.float64)
    on_sphere = pg.perm.cpu().numpy() < n_sphere
    d, nb = cKDTree(x64).query(x64, k=knn + 1)
    a, b = d[:, knn - 1] ** 2, d[:, knn] ** 2
    tie = b <= a * (1.0 + 4e-6)
    p = x64[nb[:, :knn]]
    c = p - p.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum('nki,nkj->nij', c, c))
    good = (w[:, 1] - w[:, 0]) / w[:, 2] > 1e-2
    assert good[on_sphere].mean() > 0.99
    res = {}
    for name in ('handed_back', 'thread_only'):
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
        r2 = torch.empty(n, dtype=torch.float32, device=dev)
        valid = torch.empty(n, dtype=torch.int32, device=dev)
        todo = torch.full((n,), -1, dtype=torch.int32, device=dev) if name == 'handed_back' else None
        call('nksr_knn_pca_normals', ptr(pg.xyz), n, *_grid_args(pg), knn, 6, ptr(nrm), ptr(r2), ptr(valid), ptr(todo), stream())
        res[name] = (r2, valid)
        if todo is not None:
            assert set(np.unique(todo.cpu().numpy()).tolist()) == todo_values
        assert bool((valid > 0).all())
        r = r2.cpu().numpy().astype(np.float64)
        pu.check('normals[%s,%s]:r2_vs_exact_kth' % (case, name), (np.abs(r - a) / a).max(), 4e-7)
        assert (r[~tie] < b[~tie]).all() and (r >= a * (1 - 4e-7)).all()
        ang = np.linalg.norm(np.cross(nrm.cpu().numpy().astype(np.float64), v[:, :, 0]), axis=1)
        pu.check('normals[%s,%s]:normal_angle_well_conditioned' % (case, name), ang[good].max(), 2e-5)
    pu.report('normals[%s]:near_ties' % case, fraction=float(tie.mean()))
    assert torch.equal(res['handed_back'][1], res['thread_only'][1])
    assert torch.equal(res['handed_back'][0].view(torch.int32), res['thread_only'][0].view(torch.int32))


def test_preprocess_fn_drives_reconstruct():
    """sensor-only input through reconstruct(..., preprocess_fn=...) (examples/recons_waymo.py:30-37)."""
    import nksr
    from nksr_amd import utils
    dev = torch.device('cuda:0')
    xyz, _ = utils.synth_sphere(6000, 0.45, 0.002, seed=1)
    sensor = np.zeros_like(xyz)                              # scanner at the centre: normals point inward
    rec = nksr.Reconstructor(dev)
    field = rec.reconstruct(torch.from_numpy(xyz).to(dev), sensor=torch.from_numpy(sensor).to(dev), voxel_size=0.05,
                            approx_kernel_grad=True, solver_tol=1e-4, fused_mode=True,
                            preprocess_fn=nksr.get_estimate_normal_preprocess_fn(32, 85.0))
    mesh = field.extract_dual_mesh(mise_iter=1)
    r = np.linalg.norm(mesh.v.cpu().numpy(), axis=1)
    assert abs(np.median(r) - 0.45) < 0.01
    # inward-facing normals => the "inside" (f>0) is the OUTSIDE of the sphere
    f = field.evaluate_f(torch.tensor([[0.0, 0.0, 0.0], [0.6, 0.0, 0.0]], device=dev)).value.cpu().numpy()
    assert f[0] <= 0 < f[1] or f[0] < 0 <= f[1]


def test_pcnn_field_nearest_colour():
    import nksr
    from scipy.spatial import cKDTree
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    ref = rs.rand(30000, 3).astype(np.float32)
    col = rs.rand(30000, 3).astype(np.float32)
    q = (rs.rand(5000, 3).astype(np.float32) - 0.1) * 1.2   # some queries outside the cloud's box
    fld = nksr.fields.PCNNField(torch.from_numpy(ref).to(dev), torch.from_numpy(col).to(dev))
    c = fld.evaluate_color(torch.from_numpy(q).to(dev)).cpu().numpy()
    d, j = cKDTree(ref).query(q)
    same = (c == col[j]).all(1)
    # ties between equidistant points may pick another index; distances must still be minimal
    assert same.mean() > 0.999
