"""Moving-least-squares projection on the GPU (csrc/mls.hip k_mls_project; nksr_amd/mls.py) against the float64 restatement
tests/mls_ref.py, whose own accuracy and whose conditions on these very inputs tests/test_mls_cpu.py asserts without a GPU.

Bounds.  Agreement with the restatement: both sides sum at most 90 float64 terms per entry (different order: rounding ~1e-15 relative),
amplified by the condition number of the 6 x 6 system, which test_mls_cpu.py holds to <= 1e3 on the sphere and the plane: ~1e-11, so
positions agree within 1e-10 h, normals within 1e-10, curvatures and variation within 1e-9 of their largest magnitude.  On the lattice
cloud (volumetric blobs, up to 226 neighbours, condition numbers up to 6e7) the same rule is applied per row: the bounds times
max(cond / 1e3, 1) x max(count / 90, 1)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mls_ref as M
import segment_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('position', 'normal', 'mean_curvature', 'gaussian_curvature', 'variation', 'count', 'order_used')


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cloud():
    from nksr_amd import cloud
    return cloud


def _np(r):
    return {f: getattr(r, f).cpu().numpy() for f in FIELDS}


def _same_bits(a, b, rows=slice(None)):
    for f in FIELDS:
        x, y = getattr(a, f)[rows], getattr(b, f)[rows]
        assert x.dtype == y.dtype and x.shape == y.shape, f
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), f


def _finite_or_nan(out):
    for f in FIELDS[:5]:
        assert not np.isinf(out[f]).any(), f


def _agree(out, ref, h, what, scale=None, curvature=True, up_to_sign=False):
    """count and order_used exactly; NaN where and only where the restatement has NaN; positions within 1e-10 h, normals within 1e-10,
    and with ``curvature`` the curvatures and the variation within 1e-9 of their largest magnitude.  ``scale`` [Q]: a factor >= 1 on
    every row's bound.  ``up_to_sign``: every row's normal and mean curvature are compared after giving them the restatement's sign (a
    lattice cloud without input normals: two components of a normal can tie exactly, and which of them counts as the larger hangs on a
    rounding; positions, Gaussian curvature and variation do not depend on the sign).  Prints and returns the measured maxima."""
    if up_to_sign:
        sign = np.where(np.nan_to_num((out['normal'] * ref['normal']).sum(1)) < 0, -1.0, 1.0)
        out = dict(out, normal=out['normal'] * sign[:, None], mean_curvature=out['mean_curvature'] * sign)
    assert np.array_equal(out['count'], ref['count']), what
    assert np.array_equal(out['order_used'], ref['order_used']), what
    for f in FIELDS[:5]:
        assert np.array_equal(np.isnan(out[f]), np.isnan(ref[f])), (what, f)
    scale = np.ones(len(out['count'])) if scale is None else scale
    dp = np.abs(out['position'] - ref['position']).max(1) / h
    dn = np.nan_to_num(np.abs(out['normal'] - ref['normal']).max(1))
    got = {'position / h': float(dp.max()), 'normal': float(dn.max())}
    for f in FIELDS[2:5]:
        if np.isfinite(ref[f]).any():
            got[f + ' (rel)'] = float(np.nanmax(np.abs(out[f] - ref[f])) / np.nanmax(np.abs(ref[f])))
    print('%s: %s' % (what, ', '.join('%s %.3g' % kv for kv in got.items())))
    assert (dp <= 1e-10 * scale).all() and (dn <= 1e-10 * scale).all(), (what, got)
    if curvature:
        for f in FIELDS[2:5]:
            assert got.get(f + ' (rel)', 0.0) <= 1e-9 * scale.max(), (what, f, got)
    return got


# ---- 4. agreement with the restatement on the noisy sphere -----------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('with_normal', [True, False])
def test_sphere_matches_the_restatement(order, with_normal):
    xyz, nrm = M.noisy_sphere()
    ref = M.sphere_ref(order, with_normal)
    index = _cloud().CloudIndex(_gpu(xyz))
    r = index.mls_project(M.SPHERE_H, normal=_gpu(nrm) if with_normal else None, order=order)
    assert r.position.dtype == torch.float64 and r.count.dtype == torch.int32 and r.order_used.dtype == torch.int8 and r.valid.dtype == torch.bool
    assert r.xyz.dtype == torch.float32 and r.normal32.dtype == torch.float32 and tuple(r.position.shape) == (len(xyz), 3)
    assert torch.equal(r.count, index.radius_count(M.SPHERE_H))
    assert torch.equal(r.valid, r.order_used > 0) and bool(r.valid.all())
    _agree(_np(r), ref, M.SPHERE_H, 'sphere order %d %s normals' % (order, 'with' if with_normal else 'without'))
    if order == 1:
        assert bool(torch.isnan(r.mean_curvature).all()) and bool(torch.isnan(r.gaussian_curvature).all())
    if with_normal:
        assert float((r.normal * _gpu(nrm).double()).sum(1).min()) > 0.9


# ---- 5. reproduction of a plane ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2])
def test_plane_is_reproduced(order):
    """The only error is the float32 rounding of the inputs: the bound is four times what the restatement's own outputs are off by."""
    xyz, query = M.tilted_plane()
    ref = M.mls_project(xyz, M.PLANE_H, query=query, order=order)
    assert (ref['order_used'] == order).all()
    r = _cloud().mls_project(_gpu(xyz), M.PLANE_H, query=_gpu(query), order=order)
    out = _np(r)
    assert (out['order_used'] == order).all() and np.array_equal(out['count'], ref['count'])
    dist, ref_dist = np.abs(M.plane_distance(out['position'])).max(), np.abs(M.plane_distance(ref['position'])).max()
    tilt = np.linalg.norm(np.cross(out['normal'], M.PLANE_NORMAL), axis=1).max()
    ref_tilt = np.linalg.norm(np.cross(ref['normal'], M.PLANE_NORMAL), axis=1).max()
    print('plane order %d: distance %.3g (restatement %.3g), normal tilt %.3g (restatement %.3g)' % (order, dist, ref_dist, tilt, ref_tilt))
    assert dist <= 4 * ref_dist and tilt <= 4 * ref_tilt
    assert (np.abs(out['normal'] @ M.PLANE_NORMAL) > 0.999999).all()
    # the queries moved along the normal only: their in-plane position is kept to the same bound
    moved = out['position'] - query.astype(np.float64)
    assert np.abs(moved - (moved @ M.PLANE_NORMAL)[:, None] * M.PLANE_NORMAL).max() <= 4 * ref_dist + 0.3 * M.PLANE_H * 4 * ref_tilt
    if order == 2:
        curv, ref_curv = np.abs(out['mean_curvature']).max(), np.abs(ref['mean_curvature']).max()
        print('plane order 2: |mean curvature| %.3g (restatement %.3g)' % (curv, ref_curv))
        assert curv <= 4 * ref_curv
    _agree(out, ref, M.PLANE_H, 'plane order %d vs restatement' % order, curvature=False)     # (curvature, variation ~ 0: held above)


# ---- 6. the radius is inclusive and fp32 ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _lattice():
    k = S.lattice_cloud()
    return k, S.lattice_xyz(k), M.LATTICE_R * S.UNIT


@pytest.mark.parametrize('order', [1, 2])
def test_lattice_pairs_exactly_at_the_radius_count(order):
    k, xyz, h = _lattice()
    assert S.lattice_pairs(k, M.LATTICE_R)[1] > 100                    # pairs EXACTLY at the radius exist
    ref = M.mls_project(xyz, h, order=order)
    exact = 1 + np.bincount(S.lattice_pairs(k, M.LATTICE_R)[0].ravel(), minlength=len(k))
    assert np.array_equal(ref['count'], exact)                         # the restatement's neighbour set is the integer one
    index = _cloud().CloudIndex(_gpu(xyz))
    r = index.mls_project(h, order=order)
    assert torch.equal(r.count, index.radius_count(h))
    out = _np(r)
    _finite_or_nan(out)
    cond = np.where(np.isfinite(ref['cond']), ref['cond'], 1.0)
    scale = np.maximum(cond / 1e3, 1.0) * np.maximum(ref['count'] / 90.0, 1.0)
    _agree(out, ref, h, 'lattice order %d' % order, scale=scale, up_to_sign=True)


# ---- 7. degenerate inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(M.degenerate_clouds()))
def test_degenerate_inputs(name):
    xyz, h, order, expect = M.degenerate_clouds()[name]
    xyz = xyz.astype(np.float32)
    ref = M.mls_project(xyz, h, order=order)
    r = _cloud().mls_project(_gpu(xyz), h, order=order)
    out = _np(r)
    _finite_or_nan(out)
    assert np.array_equal(out['order_used'], ref['order_used']) and np.array_equal(out['count'], ref['count'])
    if expect is not None:
        assert out['order_used'][0] == expect
        assert np.array_equal(out['position'][0], xyz[0].astype(np.float64))                 # unchanged, to the bit
        assert np.isnan(out['mean_curvature'][0]) and np.isnan(out['gaussian_curvature'][0]) and np.isnan(out['normal'][0]).all()
        assert not bool(r.valid[0])
    if name in ('collinear', 'coincident', 'patch6', 'patch7', 'single'):
        assert (out['order_used'] == 0).all() and np.array_equal(out['position'], xyz.astype(np.float64))
    if name == 'line_plus_one':                     # the plane through the line and the one point off it: z = 0
        assert (out['order_used'] == 1).all() and np.abs(out['position'][:, 2]).max() < 1e-12 and np.isnan(out['mean_curvature']).all()
        assert np.abs(np.abs(out['normal'][:, 2]) - 1).max() < 1e-12


def test_unfitted_rows_keep_their_input_normal():
    xyz = M.degenerate_clouds()['collinear'][0].astype(np.float32)
    nrm = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (len(xyz), 1))
    r = _cloud().mls_project(_gpu(xyz), 0.5, normal=_gpu(nrm), order=1)
    assert not bool(r.valid.any()) and torch.equal(r.normal, _gpu(nrm).double()) and torch.equal(r.xyz, _gpu(xyz))


def test_empty_query_set():
    xyz, _ = M.noisy_sphere()
    r = _cloud().mls_project(_gpu(xyz[:500]), 0.25, query=torch.empty((0, 3), device='cuda'))
    assert tuple(r.position.shape) == (0, 3) and r.count.numel() == 0 and r.order_used.dtype == torch.int8 and r.valid.numel() == 0


@functools.lru_cache(None)
def _far_cloud():
    """3 000 points on a sphere of radius 0.05 about (1000, 1000, 1000) as float32 (spacing 2^-14 there), and the same points less 1000
    (exact in float32): the same geometry to the bit"""
    rs = np.random.RandomState(17)
    u = rs.randn(3000, 3)
    far = (1000.0 + 0.05 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    near = (far.astype(np.float64) - 1000.0).astype(np.float32)
    assert np.array_equal(near.astype(np.float64) + 1000.0, far.astype(np.float64))
    return far, near


def test_cloud_offset_by_a_thousand():
    far, near = _far_cloud()
    a = _cloud().mls_project(_gpu(far), 0.01, order=2)
    b = _cloud().mls_project(_gpu(near), 0.01, order=2)
    assert torch.equal(a.count, b.count) and torch.equal(a.order_used, b.order_used) and int(a.count.min()) >= 8 and bool(a.valid.all())
    spacing = 2.0 ** -14                             # of float32 at 1000
    dp = float((a.position - 1000.0 - b.position).abs().max())
    dn = float((a.normal - b.normal).abs().max())
    dh = float((a.mean_curvature - b.mean_curvature).abs().max() / b.mean_curvature.abs().max())
    print('offset 1e3: position %.3g (float32 spacing %.3g), normal %.3g, mean curvature (rel) %.3g' % (dp, spacing, dn, dh))
    assert dp <= spacing and dn <= spacing / 0.01 and dh <= spacing / 0.01


# ---- 8. determinism and lane independence ----------------------------------------------------------------------------------------------
def test_same_bits_twice_alone_and_as_explicit_queries():
    xyz, nrm = M.noisy_sphere()
    x, n = _gpu(xyz), _gpu(nrm)
    index = _cloud().CloudIndex(x)
    for order in (1, 2):
        full = index.mls_project(M.SPHERE_H, normal=n, order=order)
        _same_bits(full, index.mls_project(M.SPHERE_H, normal=n, order=order))
        explicit = index.mls_project(M.SPHERE_H, normal=n, query=x, order=order)
        _same_bits(full, explicit)
        alone = index.mls_project(M.SPHERE_H, normal=n, query=x[:100].contiguous(), order=order)
        _same_bits(alone, explicit, slice(0, 100))
        _same_bits(alone, full, slice(0, 100))


# ---- 9. smooth_mls and the preprocess function -----------------------------------------------------------------------------------------
def test_smooth_mls_is_the_chained_projection():
    cloud = _cloud()
    xyz, nrm = M.noisy_sphere()
    far = np.array([[3.0, 3.0, 3.0], [-3.0, 3.0, 0.0]], np.float32)                  # two points nothing is near: they stay put
    x0, n0 = _gpu(np.concatenate([xyz, far])), _gpu(np.concatenate([nrm, nrm[:2]]))
    for normal in (n0, None):
        x, n = x0, normal
        for _ in range(3):
            r = cloud.mls_project(x, M.SPHERE_H, normal=n)
            x = torch.where(r.valid[:, None], r.xyz, x)
            last = r.normal32
            if n is not None:
                n = torch.where(r.valid[:, None], r.normal32, n)
        sx, sn = cloud.smooth_mls(x0, M.SPHERE_H, normal=normal, iterations=3)
        assert sx.dtype == torch.float32 and sn.dtype == torch.float32
        assert torch.equal(sx, x)
        want = n if normal is not None else last
        assert torch.equal(sn.view(torch.int32), want.view(torch.int32))
        assert torch.equal(sx[-2:], x0[-2:]) and not torch.equal(sx[:-2], x0[:-2])
        if normal is not None:
            assert torch.equal(sn[-2:], n0[-2:])
    rad = torch.linalg.norm(sx[:-2].double(), dim=1) - 1.0
    rad0 = torch.linalg.norm(x0[:-2].double(), dim=1) - 1.0
    print('smooth_mls x 3: RMS radial error %.4g -> %.4g' % (float(rad0.pow(2).mean().sqrt()), float(rad.pow(2).mean().sqrt())))
    assert float(rad.pow(2).mean().sqrt()) < float(rad0.pow(2).mean().sqrt())


def test_preprocess_fn_composes_and_passes_the_sensor_through():
    import nksr
    xyz, nrm = M.noisy_sphere()
    x, n = _gpu(xyz), _gpu(nrm)
    sensor = torch.zeros_like(x)
    fn = nksr.get_mls_smooth_preprocess_fn(M.SPHERE_H, order=2, iterations=2)
    out = fn(x, n, sensor)
    assert len(out) == 3 and out[2] is sensor and out[0].shape == x.shape and out[1].shape == n.shape
    sx, sn = nksr.cloud.smooth_mls(x, M.SPHERE_H, normal=n, iterations=2)
    assert torch.equal(out[0], sx) and torch.equal(out[1], sn)
    assert fn(x, None, None)[1:] == (None, None)
    both = nksr.compose_preprocess_fns(nksr.get_voxel_downsample_preprocess_fn(0.05), fn)
    out = both(x, n, None)
    assert len(out) == 3 and out[2] is None and 0 < out[0].shape[0] < x.shape[0] and out[1].shape == out[0].shape


def test_reconstruction_through_the_preprocess_fn_is_closer_to_the_sphere():
    """20 000 points on a sphere of radius 0.45 with noise 0.01, half the voxel size.  The radius must span enough neighbours to average
    the noise below what the solve itself averages (profiles/mls.md has the sweep: 0.04 and 0.06 make the mesh worse, 0.1 better)."""
    import nksr
    xyz, nrm = nksr.utils.synth_sphere(20000, 0.45, 0.01, seed=3)
    x, n = _gpu(xyz), _gpu(nrm)
    rms = {}
    for name, fn in (('as it comes', None), ('mls', nksr.get_mls_smooth_preprocess_fn(0.1, order=2, iterations=2))):
        field = nksr.Reconstructor(torch.device('cuda:0')).reconstruct(x, n, preprocess_fn=fn, voxel_size=0.02)
        v = field.extract_dual_mesh(mise_iter=1).v
        rms[name] = float((torch.linalg.norm(v.double(), dim=1) - 0.45).pow(2).mean().sqrt())
        assert v.shape[0] > 1000
    print('RMS radial error of the mesh vertices: as it comes %.5g, through get_mls_smooth_preprocess_fn %.5g' % (rms['as it comes'], rms['mls']))
    assert rms['mls'] < rms['as it comes']


# ---- 10. the example -----------------------------------------------------------------------------------------------------------------
def test_recons_denoised_example(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'recons_denoised.py')], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    print(out.stdout)
    assert (tmp_path / 'recons_denoised.ply').exists() and 'V=' in out.stdout and out.stdout.rstrip().endswith('recons_denoised.ply')
