"""nksr.cloud.icp / evaluate_registration / icp_multiscale / apply_transform on the GPU against the float64 restatement
(tests/register_ref.py).  Standard inputs: rounded box, 6 000 target points, two 4 000-point sources moved by the inverse of a known
pose T* (5 degrees, ~0.03 translation), radius 0.05.

Measured on one MI355X (printed by the tests, -s):
    convergence, source B point : 11 updates, error 1.352e-8 deg / 1.612e-10 -- the restatement's figures digit for digit
    convergence, source B plane :  4 updates, error 3.409e-8 deg / 2.853e-10 -- likewise
    convergence, source A plane :  5 updates, error 5.737e-3 deg / 3.428e-5  -- likewise
    one pass: 0 of 4 000 rows excluded as near-ties in all ten cases; largest |sum - fp64 sum| / sum |terms| = 1.0e-14 (bound 1e-12)
    15 degree start: multiscale 5.737e-3 deg / 3.428e-5; single scale at radius 0.05 reaches the same pose on this shape
    the example at 12 000 points per scan: chamfer-L1 0.01370 unregistered, 0.00239 registered"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import register_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ['point', 'plane']


def _dev():
    return torch.device('cuda:0')


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@functools.lru_cache(maxsize=None)
def std():
    """the standard inputs on the device, one CloudIndex over the target for every test, and the restatement's runs"""
    from nksr_amd import cloud
    d = R.standard_inputs()
    out = {k: _gpu(d[k]) for k in ('target', 'normal', 'source_a', 'source_b')}
    out['index'] = cloud.CloudIndex(out['target'])
    out['centre'] = R.bbox_centre(d['target'])
    assert np.array_equal(out['index'].bbox_centre(), out['centre'])
    return out


@functools.lru_cache(maxsize=None)
def ref_run(src, method):
    d = R.standard_inputs()
    return R.icp(d[src], d['target'], R.RADIUS, method=method, normal=d['normal'])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. one pass ---------------------------------------------------------------------------------------------------------------------
def _poses():
    return {'identity': np.eye(4), 'tstar': R.T_STAR, 'mid': ref_run('source_a', 'plane')['history'][2]}


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('src,pose', [('source_a', 'identity'), ('source_a', 'tstar'), ('source_a', 'mid'), ('source_b', 'tstar'),
                                      ('source_b', 'identity')])
def test_one_pass_correspondences_and_sums(method, src, pose):
    from nksr_amd import cloud
    g, d, T = std(), R.standard_inputs(), _poses()[pose]
    res = cloud.evaluate_registration(g[src], g['index'], R.RADIUS, transformation=T, method=method, target_normal=g['normal'])
    corr = res.correspondence_set.cpu().numpy()
    assert res.correspondence_set.dtype == torch.int64 and res.correspondence_set.is_cuda and corr.shape == (4000,)
    p = R.transform(T, d[src])
    idx, d1, d2 = R.nearest_within(p, d['target'], R.RADIUS)
    ok = R.decided(d1, d2, R.RADIUS)
    got = res.pass_sums[0]
    t = R.terms(method, p, d['target'], corr, g['centre'], d['normal'])
    want, scale = t.sum(0), np.abs(t).sum(0)
    rel = np.abs(got - want) / np.maximum(scale, 1e-300)
    print('%s %s %s: excluded %d of %d rows, fitness %.4f, worst |sum - fp64 sum| / sum |terms| = %.2e' % (
        method, src, pose, int((~ok).sum()), len(ok), res.fitness, rel.max()))
    assert (~ok).mean() <= 0.01
    assert np.array_equal(corr[ok], idx[ok])
    assert got[R.COUNT] == float((corr >= 0).sum()) and res.fitness == (corr >= 0).mean()
    assert (np.abs(got - want) <= 1e-12 * scale).all()
    assert (got[scale == 0] == 0).all()                                     # the fields the method does not use
    m = corr >= 0
    rmse = np.sqrt(((p[m] - d['target'].astype(np.float64)[corr[m]]) ** 2).sum() / m.sum())
    assert abs(res.inlier_rmse - rmse) <= 1e-12 * rmse
    assert res.iterations == 0 and not res.converged and np.array_equal(res.transformation.numpy(), T)


# ---- 2. bitwise repeatability --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
def test_icp_twice_gives_the_same_bits(method):
    from nksr_amd import cloud
    g = std()
    a = cloud.icp(g['source_a'], g['target'], R.RADIUS, method=method, target_normal=g['normal'], max_iteration=8)
    b = g['index'].icp(g['source_a'], R.RADIUS, method=method, target_normal=g['normal'], max_iteration=8)
    assert len(a.pass_sums) == len(b.pass_sums) >= 2
    for x, y in zip(a.pass_sums, b.pass_sums):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.array_equal(_bits(a.transformation.numpy()), _bits(b.transformation.numpy()))
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and a.iterations == b.iterations
    assert torch.equal(a.correspondence_set, b.correspondence_set)


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
def test_duplicated_target_keeps_the_lower_index_and_the_sums(method):
    from nksr_amd import cloud
    g = std()
    n = g['target'].shape[0]
    T = _poses()['mid']
    plain = cloud.evaluate_registration(g['source_a'], g['index'], R.RADIUS, T, method=method, target_normal=g['normal'])
    twice = cloud.evaluate_registration(g['source_a'], torch.cat([g['target'], g['target']]), R.RADIUS, T, method=method,
                                        target_normal=torch.cat([g['normal'], g['normal']]))
    assert twice.fitness == 1.0 and int(twice.correspondence_set.min()) >= 0 and int(twice.correspondence_set.max()) < n
    assert torch.equal(twice.correspondence_set, plain.correspondence_set)
    assert np.array_equal(_bits(twice.pass_sums[0]), _bits(plain.pass_sums[0]))


# ---- 4. convergence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('src,method,factor,slack', [('source_b', 'point', 4.0, 1e-7), ('source_b', 'plane', 4.0, 1e-7),
                                                     ('source_a', 'plane', 2.0, 0.0)])
def test_icp_converges_to_the_pose(src, method, factor, slack):
    """Source B (a subset of the target): at most 4 x the restatement's own error + 1e-7 (one fp32 ulp of coordinates of this size;
    the rotation error in radians, which is the displacement it causes at unit distance).  Source A (fresh samples): at most 2 x the
    restatement's error -- flipped near-tie correspondences move the estimate by less than the sampling error."""
    g = std()
    res = g['index'].icp(g[src], R.RADIUS, method=method, target_normal=g['normal'], max_iteration=30)
    ref = ref_run(src, method)
    rot, trans = R.pose_error(res.transformation.numpy())
    rot_ref, trans_ref = R.pose_error(ref['transformation'])
    print('%s %s: GPU %d updates, rotation error %.4g deg, translation error %.4g; restatement %d updates, %.4g deg, %.4g' % (
        src, method, res.iterations, np.degrees(rot), trans, ref['iterations'], np.degrees(rot_ref), trans_ref))
    assert res.converged and res.iterations <= 30 and res.fitness == 1.0
    assert rot <= factor * rot_ref + slack and trans <= factor * trans_ref + slack


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------------------------
def _assert_nothing_found(res, init, n):
    assert res.fitness == 0.0 and res.inlier_rmse == 0.0 and not res.converged and res.iterations == 0
    assert np.array_equal(res.transformation.numpy(), init)
    assert res.correspondence_set.shape == (n,) and bool((res.correspondence_set == -1).all())
    assert len(res.pass_sums) == 1 and not res.pass_sums[0].any()


@pytest.mark.parametrize('method', METHODS)
def test_nothing_within_the_radius(method):
    g = std()
    res = g['index'].icp(g['source_a'] + 10.0, R.RADIUS, method=method, target_normal=g['normal'])
    _assert_nothing_found(res, np.eye(4), 4000)
    far = np.eye(4)
    far[:3, 3] = [1e9, -1e9, 1e9]                                          # far outside the key range of the grid
    _assert_nothing_found(g['index'].icp(g['source_a'], R.RADIUS, init=far, method=method, target_normal=g['normal']), far, 4000)
    far[:3, 3] = [1e300, 0.0, 0.0]                                         # fl32(p) overflows
    _assert_nothing_found(g['index'].icp(g['source_a'], R.RADIUS, init=far, method=method, target_normal=g['normal']), far, 4000)


def test_single_points_and_too_few_correspondences():
    from nksr_amd import cloud
    one_t, one_s = _gpu(np.array([[0.1, 0.2, 0.31]], np.float32)), _gpu(np.array([[0.1, 0.2, 0.3]], np.float32))
    nrm = _gpu(np.array([[0.0, 0.0, 1.0]], np.float32))
    for method in METHODS:
        res = cloud.icp(one_s, one_t, 0.05, method=method, target_normal=nrm)
        assert res.fitness == 1.0 and res.correspondence_set.tolist() == [0] and abs(res.inlier_rmse - 0.01) < 1e-7
        assert not res.converged and res.iterations == 0 and np.array_equal(res.transformation.numpy(), np.eye(4))
    # two correspondences only (the other source points are out of reach): degenerate, no update
    d = R.standard_inputs()
    src = np.concatenate([d['target'][:2] + np.float32(0.001), d['target'][:3] + np.float32(5.0)])
    g = std()
    for method in METHODS:
        res = g['index'].icp(_gpu(src), 0.01, method=method, target_normal=g['normal'])
        assert res.fitness == 2 / 5 and res.correspondence_set.tolist() == [0, 1, -1, -1, -1]
        assert not res.converged and res.iterations == 0 and np.array_equal(res.transformation.numpy(), np.eye(4))


def test_a_point_at_exactly_the_radius_counts():
    from nksr_amd import cloud
    target = _gpu(np.array([[0.0, 0.0, 0.0], [3.0, 3.0, 3.0]], np.float32))
    just_out = np.nextafter(np.float32(0.5), np.float32(1.0))
    src = _gpu(np.array([[0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [0.0, 0.0, 0.5], [0.0, -0.5, 0.0], [just_out, 0.0, 0.0], [0.0, -just_out, 0.0]],
                        np.float32))
    res = cloud.evaluate_registration(src, target, 0.5)
    assert res.correspondence_set.tolist() == [0, 0, 0, 0, -1, -1] and res.fitness == 4 / 6 and res.inlier_rmse == 0.5


def test_argument_checks():
    from nksr_amd import cloud
    g = std()
    with pytest.raises(RuntimeError):
        g['index'].icp(g['source_a'].cpu(), R.RADIUS)                                  # another device
    with pytest.raises(RuntimeError):
        g['index'].icp(g['source_a'].long(), R.RADIUS)                                 # another dtype
    with pytest.raises(RuntimeError):
        g['index'].icp(g['source_a'][:, :2], R.RADIUS)
    with pytest.raises(ValueError):
        g['index'].icp(g['source_a'][:0], R.RADIUS)
    with pytest.raises(ValueError):
        cloud.icp(g['source_a'], g['target'][:0], R.RADIUS)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            g['index'].icp(g['source_a'], r)
    with pytest.raises(ValueError):
        g['index'].icp(g['source_a'], R.RADIUS, method='plane')
    with pytest.raises(RuntimeError):
        g['index'].icp(g['source_a'], R.RADIUS, method='plane', target_normal=g['normal'][:10])
    with pytest.raises(ValueError):
        g['index'].icp(g['source_a'], R.RADIUS, method='colored')
    with pytest.raises(ValueError):
        g['index'].icp(g['source_a'], R.RADIUS, init=np.eye(3))
    with pytest.raises(ValueError):
        g['index'].icp(g['source_a'], R.RADIUS, init=2.0 * np.eye(4))


# ---- 6. the other entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
def test_evaluate_registration_is_pass_zero_of_icp(method):
    from nksr_amd import cloud
    g = std()
    T = _poses()['mid']
    ev = cloud.evaluate_registration(g['source_a'], g['target'], R.RADIUS, T, method=method, target_normal=g['normal'])
    run = cloud.icp(g['source_a'], g['target'], R.RADIUS, init=T, method=method, target_normal=g['normal'], max_iteration=3)
    none = cloud.icp(g['source_a'], g['target'], R.RADIUS, init=T, method=method, target_normal=g['normal'], max_iteration=0)
    assert np.array_equal(_bits(ev.pass_sums[0]), _bits(run.pass_sums[0])) and np.array_equal(_bits(ev.pass_sums[0]), _bits(none.pass_sums[0]))
    assert (ev.fitness, ev.inlier_rmse) == (none.fitness, none.inlier_rmse) and torch.equal(ev.correspondence_set, none.correspondence_set)
    assert none.iterations == 0 and not none.converged and len(none.pass_sums) == 1
    assert run.iterations == len(run.pass_sums) - 1          # the last pass evaluates the transformation that is returned


def test_multiscale_from_a_wide_start():
    from nksr_amd import cloud
    g = std()
    init = R.rigid((-1.0, 1.0, 2.0), 15.0) @ R.T_STAR
    multi = cloud.icp_multiscale(g['source_a'], g['target'], [0.08, 0.04, None], [0.2, 0.1, R.RADIUS], [30, 30, 30], init=init,
                                 method='plane', target_normal=g['normal'])
    single = cloud.icp(g['source_a'], g['target'], R.RADIUS, init=init, method='plane', target_normal=g['normal'])
    rot_ref, trans_ref = R.pose_error(ref_run('source_a', 'plane')['transformation'])
    rot, trans = R.pose_error(multi.transformation.numpy())
    rot_s, trans_s = R.pose_error(single.transformation.numpy())
    print('15 degree start: multiscale %.4g deg / %.4g (converged %s), single scale %.4g deg / %.4g (converged %s); restatement from '
          'identity %.4g deg / %.4g' % (np.degrees(rot), trans, multi.converged, np.degrees(rot_s), trans_s, single.converged,
                                        np.degrees(rot_ref), trans_ref))
    assert multi.converged and rot <= 2.0 * rot_ref and trans <= 2.0 * trans_ref
    assert multi.correspondence_set.shape == (4000,) and multi.fitness == 1.0


def test_apply_transform_against_float64_numpy():
    from nksr_amd import cloud
    g, d = std(), R.standard_inputs()
    T = R.rigid((3.0, -1.0, 2.0), 37.0, (100.0, -0.25, 3e-3))
    xyz, nrm = cloud.apply_transform(g['source_a'], T, g['normal'][:4000])
    want = d['source_a'].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    want_n = d['normal'][:4000].astype(np.float64) @ T[:3, :3].T
    assert xyz.dtype == torch.float32 and nrm.dtype == torch.float32
    assert (np.abs(xyz.cpu().numpy() - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert (np.abs(nrm.cpu().numpy() - want_n) <= np.spacing(np.abs(want_n).astype(np.float32))).all()
    assert torch.equal(cloud.apply_transform(g['source_a'], np.eye(4)), g['source_a'])


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------------
def test_recons_registered_example(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'recons_registered.py'), '12000'], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    print(out.stdout)
    last = out.stdout.strip().splitlines()[-1].split()
    raw, reg = float(last[1].split('=')[1]), float(last[2].split('=')[1])
    assert (tmp_path / 'recons_registered.ply').exists() and reg < raw
