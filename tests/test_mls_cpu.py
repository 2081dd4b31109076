"""Moving-least-squares projection without a GPU: the restatement (tests/mls_ref.py) against analytic truth, the conditions on the
inputs that tests/test_gpu_mls.py relies on -- asserted here on the restatement alone, before a GPU is involved --, and the Python
surface rejecting bad arguments before a device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mls_ref as M
import segment_ref as S


def _radial(p, r=1.0):
    d = np.linalg.norm(np.asarray(p, np.float64), axis=1) - r
    return float(np.sqrt((d * d).mean())), float(d.mean())


# ---- 1. the restatement against analytic truth ----------------------------------------------------------------------------------------
def test_projection_denoises_a_sphere_and_order_two_shrinks_less():
    """Measured when this test was written (4 000 points on the unit sphere, Gaussian noise 0.01, h = 0.25, sigma = h / 2; 38 - 86
    neighbours): RMS radial error 0.00997 of the input, 0.00317 after one order-2 projection (mean -0.00015), 0.00725 after one order-1
    projection (mean -0.00693: the plane cuts the cap off); the fitted normals are 1.38 degrees (order 2) and 1.54 degrees (order 1)
    off the true ones on average.  Every bound below is twice the measured figure."""
    xyz, nrm = M.noisy_sphere()
    rms_in, _ = _radial(xyz)
    rms1, bias1 = _radial(M.sphere_ref(1, True)['position'])
    rms2, bias2 = _radial(M.sphere_ref(2, True)['position'])
    ang = [float(np.degrees(np.arccos(np.clip((M.sphere_ref(o, True)['normal'] * nrm).sum(1), -1, 1))).mean()) for o in (1, 2)]
    print('RMS radial error: input %.5f, order 1 %.5f (mean %.5f), order 2 %.5f (mean %.5f); normals off by %.3f / %.3f degrees'
          % (rms_in, rms1, bias1, rms2, bias2, ang[0], ang[1]))
    assert 0.009 < rms_in < 0.011
    assert rms2 < rms_in and rms2 <= 2 * 0.00317
    assert rms1 <= 2 * 0.00725 and abs(bias1) <= 2 * 0.00693
    assert abs(bias2) <= 2 * 0.00015 and abs(bias2) < abs(bias1)
    assert ang[1] <= 2 * 1.38 and ang[0] <= 2 * 1.54
    for o in (1, 2):
        v = M.sphere_ref(o, True)['variation']
        assert (v >= 0).all() and (v < 1.0 / 3).all()
    assert np.isnan(M.sphere_ref(1, True)['mean_curvature']).all()


def test_curvature_of_a_clean_unit_sphere():
    """Measured: mean curvature 1.0091 .. 1.0135 (largest |H - 1| 0.0135), Gaussian 1.0182 .. 1.0272 (largest |K - 1| 0.0272): the quadric
    over a cap of h = 0.25 overestimates by O(h^2); the projected points are 3.2e-5 (RMS) off the sphere.  Bounds: twice those.  The sign follows the normals handed in."""
    xyz, nrm = M.clean_sphere()
    r = M.mls_project(xyz, M.SPHERE_H, normal=nrm, order=2)
    H, K = r['mean_curvature'], r['gaussian_curvature']
    print('clean sphere: H %.4f .. %.4f, K %.4f .. %.4f' % (H.min(), H.max(), K.min(), K.max()))
    assert (r['order_used'] == 2).all()
    assert np.abs(H - 1).max() <= 2 * 0.0135 and np.abs(K - 1).max() <= 2 * 0.0272
    assert _radial(r['position'])[0] <= 2 * 3.2e-5
    flipped = M.mls_project(xyz, M.SPHERE_H, normal=-nrm, order=2)
    assert np.allclose(flipped['mean_curvature'], -H, rtol=0, atol=1e-12) and np.allclose(flipped['gaussian_curvature'], K, rtol=0, atol=1e-12)
    assert np.allclose(flipped['position'], r['position'], rtol=0, atol=1e-14) and np.allclose(flipped['normal'], -r['normal'], rtol=0, atol=1e-14)


def test_the_result_does_not_depend_on_the_frame_within_the_plane():
    """u, v turned by 0.7 rad (and the sums taken in another order by einsum): positions move by 1e-15 h (measured 9e-16)."""
    xyz, nrm = M.noisy_sphere()
    a, b = M.sphere_ref(2, True), M.mls_project(xyz, M.SPHERE_H, normal=nrm, order=2, rotate_frame=0.7)
    assert np.abs(a['position'] - b['position']).max() <= 1e-13 * M.SPHERE_H and np.abs(a['normal'] - b['normal']).max() <= 1e-13
    assert np.abs(a['mean_curvature'] - b['mean_curvature']).max() <= 1e-12


def test_hand_cases():
    # nine points of z = 0.5 (x^2 + y^2), symmetric about both axes, so the fitted plane is horizontal and the quadric over it exact
    pts = np.array([[0, 0], [0.3, 0], [0, 0.3], [-0.3, 0], [0, -0.3], [0.2, 0.2], [-0.2, 0.2], [0.2, -0.2], [-0.2, -0.2]], float)
    xyz = np.concatenate([pts, 0.5 * (pts ** 2).sum(1, keepdims=True)], 1)
    r = M.mls_project(xyz, 1.0, normal=np.tile([[0, 0, 1.0]], (9, 1)), query=np.zeros((1, 3)), order=2, min_neighbors=6)
    assert r['order_used'][0] == 2 and r['count'][0] == 9
    assert np.abs(r['position'][0]).max() < 1e-7 and abs(r['normal'][0, 2] - 1) < 1e-7             # (float32 inputs)
    assert abs(r['mean_curvature'][0] + 1.0) < 1e-6 and abs(r['gaussian_curvature'][0] - 1.0) < 1e-6   # a cup seen from above: H = -1
    # without normals the largest component is made positive
    r = M.mls_project(xyz * [1, 1, -1], 1.0, query=np.zeros((1, 3)), order=2, min_neighbors=6)
    assert r['normal'][0, 2] > 0.99 and abs(r['mean_curvature'][0] - 1.0) < 1e-6
    # the radius is inclusive: a point exactly h away counts
    line = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]], np.float32)
    assert M.mls_project(line, 0.25, order=1)['count'].tolist() == [2, 3, 2]


# ---- 2. the conditions the GPU tests rest on ------------------------------------------------------------------------------------------
def test_conditions_on_the_noisy_sphere():
    """Measured: 38 - 86 neighbours, condition number at most 239, l0 / l1 at most 0.058, |sum w n_i . n| / W at least 0.989, the pair
    nearest the radius 2.9e-6 (relative) from it."""
    xyz, nrm = M.noisy_sphere()
    r = M.sphere_ref(2, True)
    print('sphere: count %d - %d, cond %.0f, l0/l1 %.3f, sign margin %.3f' % (r['count'].min(), r['count'].max(), r['cond'].max(),
                                                                                r['eig_ratio'].max(), r['sign_margin'].min()))
    assert r['count'].min() >= 30 and r['count'].max() <= 90
    assert (r['order_used'] == 2).all() and r['cond'].max() <= 1e3 and r['eig_ratio'].max() <= 0.2
    assert r['sign_margin'].min() >= 1e-3
    assert M.radius_gap(xyz, xyz, M.SPHERE_H) >= 1e-6
    # without normals: no sign hangs on which of two components is the larger
    n = np.sort(np.abs(M.sphere_ref(2, False)['normal']), axis=1)
    assert (n[:, 2] - n[:, 1]).min() >= 1e-9
    assert np.array_equal(M.sphere_ref(1, True)['count'], r['count']) and (M.sphere_ref(1, False)['order_used'] == 1).all()


def test_conditions_on_the_tilted_plane():
    """Measured: 79 - 97 neighbours, condition number 101; the float32 inputs lie within 1.7e-8 of the plane, the restatement's outputs
    within 2.2e-9 (order 1) and 4.8e-9 (order 2), its normals within 2e-8 rad, |H| <= 1.9e-6."""
    xyz, query = M.tilted_plane()
    assert len(xyz) == 2000 and len(query) == 256 and np.abs(M.plane_distance(xyz)).max() < 1e-7
    off = np.abs(M.plane_distance(query))
    assert 0.25 * M.PLANE_H < off.max() <= 0.3 * M.PLANE_H * (1 + 1e-6)
    assert M.radius_gap(xyz, query, M.PLANE_H) >= 1e-6
    for order in (1, 2):
        r = M.mls_project(xyz, M.PLANE_H, query=query, order=order)
        assert (r['order_used'] == order).all() and r['count'].min() >= 50 and r['eig_ratio'].max() <= 0.2
        d = np.abs(M.plane_distance(r['position'])).max()
        print('plane order %d: outputs within %.3g of the plane' % (order, d))
        assert 0 < d < 1e-7
        n = np.sort(np.abs(r['normal']), axis=1)
        assert (n[:, 2] - n[:, 1]).min() >= 1e-9
        if order == 2:
            assert r['cond'].max() <= 1e3 and 0 < np.abs(r['mean_curvature']).max() < 1e-4


@functools.lru_cache(None)
def _lattice(order):
    k = S.lattice_cloud()
    return k, M.mls_project(S.lattice_xyz(k), M.LATTICE_R * S.UNIT, order=order)


@pytest.mark.parametrize('order', [1, 2])
def test_conditions_on_the_lattice_cloud(order):
    """Everything the predicate meets is exact in float32 (test_segment_cpu.py: test_lattice_cloud_is_exact_in_fp32, r <= 50 units), 242
    pairs lie exactly at the radius of 25 units.  No decision hangs on a rounding: measured, the smallest Cholesky pivot ratio is 1.9e-8,
    the smallest eigenvalue gap (l1 - l0) / l2 of a fitted row 2.4e-4, the smallest l1 / l2 of a fitted row 1e-4 or more."""
    k, r = _lattice(order)
    assert S.lattice_pairs(k, M.LATTICE_R)[1] > 100
    used = r['order_used'] > 0
    assert used.sum() > 3000 and (~used).sum() > 100                # both kinds of row are there
    val = r['eigenvalues'][used]
    assert ((val[:, 1] - val[:, 0]) / val[:, 2]).min() >= 1e-4
    assert (val[:, 1] / val[:, 2]).min() >= 1e-10
    scale = r['weight'][used] * (M.LATTICE_R * S.UNIT) ** 2
    assert (val[:, 1] / scale).min() >= 1e-10                       # ... nor on the rounding floor 1e-14 W h^2
    # (symmetric neighbourhoods exist on a lattice: two components of a normal can tie exactly, and without input normals the sign
    # then hangs on a rounding -- test_gpu_mls.py compares the lattice normals up to that sign; positions do not depend on it)
    if order == 2:
        assert (r['order_used'] != 1).all() or np.nanmin(r['pivot_ratio']) >= 1e-10
        p = r['pivot_ratio'][np.isfinite(r['pivot_ratio'])]
        assert ((p >= 1e-10) | (p <= 1e-14)).all()
    # the rows that are not fitted: too few neighbours, or l1 / l2 at rounding level (exactly collinear lattice points) -- never near the threshold
    thin = ~used & np.isfinite(r['eigenvalues'][:, 0])
    ev = r['eigenvalues'][thin]
    print('lattice order %d: %d rows fitted, %d not (%d of those with enough neighbours)' % (order, used.sum(), (~used).sum(), thin.sum()))
    assert (np.abs(ev[:, 1]) <= 1e-14 * ev[:, 2]).all() and (np.abs(ev[:, 1]) <= 1e-16 * r['weight'][thin] * (M.LATTICE_R * S.UNIT) ** 2).all()


def test_conditions_on_the_degenerate_clouds():
    for name, (xyz, h, order, expect) in M.degenerate_clouds().items():
        r = M.mls_project(xyz, h, order=order)
        if expect is not None:
            assert r['order_used'][0] == expect, name
        for f in ('position', 'normal', 'mean_curvature', 'gaussian_curvature', 'variation'):
            assert not np.isinf(r[f]).any(), (name, f)
        if len(xyz) > 1:
            assert M.radius_gap(xyz, xyz, h) >= 1e-6, name
        p = r['pivot_ratio'][np.isfinite(r['pivot_ratio'])]
        assert ((p >= 1e-10) | (p <= 1e-14)).all(), (name, p.min())       # a pivot is either sound or rounding noise: the flag is safe
    r = M.mls_project(*M.degenerate_clouds()['line_plus_one'][:2], order=2)
    assert (r['order_used'] == 1).all() and np.nanmax(np.abs(r['pivot_ratio'])) <= 1e-14
    assert (M.mls_project(*M.degenerate_clouds()['patch7'][:2], order=2, min_neighbors=6)['order_used'] > 0).all()


# ---- 3. the surface, and argument errors before a device is touched --------------------------------------------------------------------
def test_surface_exists():
    import nksr
    from nksr_amd import mls
    assert nksr.cloud.mls_project is mls.mls_project and nksr.cloud.smooth_mls is mls.smooth_mls and nksr.cloud.MlsResult is mls.MlsResult
    assert callable(nksr.cloud.CloudIndex.mls_project) and callable(nksr.get_mls_smooth_preprocess_fn)
    assert 'get_mls_smooth_preprocess_fn' in nksr.__all__
    assert 'chunk_size > 0' in nksr.get_mls_smooth_preprocess_fn.__doc__
    from nksr_amd import _lib
    assert 'nksr_mls_project' in _lib.EXPORTED


class _NoDevice:
    """stands in for a CloudIndex: anything but ``n`` that is touched raises"""
    n = 10

    def __getattr__(self, name):
        raise AssertionError('the index was used (%s) before the arguments were checked' % name)


def test_bad_arguments_raise_before_any_gpu_work():
    import nksr
    cloud = nksr.cloud
    xyz, nrm = torch.zeros((10, 3)), torch.zeros((10, 3))             # CPU tensors: a call that got as far as the device check says so
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float('inf')), dict(radius=float('nan')), dict(radius=0.1, order=0),
           dict(radius=0.1, order=3), dict(radius=0.1, order=1, min_neighbors=2), dict(radius=0.1, order=2, min_neighbors=5),
           dict(radius=0.1, sigma=0.0), dict(radius=0.1, normal=torch.zeros((9, 3))), dict(radius=0.1, normal=torch.zeros((10, 2)))]
    for kw in bad:
        for what, call in (('mls_project', lambda: cloud.mls_project(xyz, **kw)), ('smooth_mls', lambda: cloud.smooth_mls(xyz, **kw)),
                           ('CloudIndex.mls_project', lambda: cloud.CloudIndex.mls_project(_NoDevice(), **kw))):
            with pytest.raises(ValueError, match='radius|order|min_neighbors|sigma|normal'):
                call()
    for it in (0, -1, 1.5):
        with pytest.raises(ValueError, match='iterations'):
            cloud.smooth_mls(xyz, 0.1, normal=nrm, iterations=it)
        with pytest.raises(ValueError, match='iterations'):
            nksr.get_mls_smooth_preprocess_fn(0.1, iterations=it)
    for kw in (dict(radius=0.0), dict(radius=0.1, order=3), dict(radius=0.1, sigma=-1.0)):
        with pytest.raises(ValueError, match='radius|order|sigma'):
            nksr.get_mls_smooth_preprocess_fn(**kw)
    # good arguments get as far as the device check, which refuses a CPU tensor
    for call in (lambda: cloud.mls_project(xyz, 0.1, normal=nrm), lambda: cloud.smooth_mls(xyz, 0.1, normal=nrm, iterations=2)):
        with pytest.raises(RuntimeError, match='GPU|cuda|MI355X'):
            call()
    with pytest.raises(RuntimeError, match='xyz'):
        cloud.mls_project(torch.zeros((10, 2)), 0.1)
    assert callable(nksr.get_mls_smooth_preprocess_fn(0.1, order=1, iterations=3, sigma=0.02))


def test_c_entry_point_rejects_bad_arguments_before_any_launch():
    from nksr_amd import _lib
    lib = _lib.lib
    one = C.c_void_p(8)                     # non-NULL, never dereferenced: every call below fails its checks

    def call(n_ref=10, hcap=8, cell=0.2, query=None, nq=5, radius=0.1, sigma=0.05, order=2, min_nb=8, out=one, grid=one):
        return lib.nksr_mls_project(grid, n_ref, grid, grid, grid, grid, hcap, cell, 1.0 / cell, None, query, nq, radius, sigma, order, min_nb,
                                    out, out, out, out, out, out, out, None)

    def err():
        return lib.nksr_last_error().decode()
    assert call(radius=0.0) != 0 and 'radius' in err()
    assert call(radius=float('inf')) != 0 and 'radius' in err()
    assert call(sigma=0.0) != 0 and 'sigma' in err()
    assert call(order=3) != 0 and 'order' in err()
    assert call(order=1, min_nb=2) != 0 and 'min_neighbors' in err()
    assert call(order=2, min_nb=5) != 0 and 'min_neighbors' in err()
    assert call(grid=None) != 0 and 'NULL' in err()
    assert call(hcap=12) != 0 and 'hcap' in err()
    assert call(cell=0.05) != 0 and 'cell' in err()
    # the words of the check that every radius search on a grid shares (csrc/knn_dev.h radius_grid_args)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        assert call(radius=r) != 0 and 'mls project: radius must be positive and finite' in err()
    assert call(hcap=12) != 0 and 'power of two' in err()
    assert call(cell=0.05) != 0 and 'must be >= radius' in err()
    assert call(nq=11) != 0 and 'n_ref' in err()
    assert call(nq=-1) != 0 and 'negative' in err()
    assert call(out=None) != 0 and 'NULL' in err()
    assert call(nq=0) == 0                  # nothing to do: no launch
