"""Registration without a GPU: the float64 restatement (tests/register_ref.py) recovers a known pose, the host-side update functions
of nksr_amd/register.py reproduce its steps from the packed sums, and the C entry points reject bad arguments before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

import register_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _register():
    from nksr_amd import register
    return register


def test_layout_constants_match_the_header():
    reg = _register()
    assert (reg.FIELDS, reg.COUNT, reg.D2, reg.PT_P, reg.PT_Q, reg.PT_PQ, reg.PL_JJ, reg.PL_JR, reg.PL_RR) == \
        (R.FIELDS, R.COUNT, R.D2, R.PT_P, R.PT_Q, R.PT_PQ, R.PL_JJ, R.PL_JR, R.PL_RR)
    assert reg.FIELDS * 8 == 256 and reg.BLOCK % 64 == 0
    from nksr_amd import build, cloud
    assert 'register.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'knn_dev.h'))
    for name in ('icp', 'icp_multiscale', 'evaluate_registration', 'apply_transform', 'IcpResult'):
        assert getattr(cloud, name) is getattr(reg, name)
    assert callable(cloud.CloudIndex.icp)


def test_standard_inputs_have_full_fitness_and_no_near_ties():
    d = R.standard_inputs()
    for src in ('source_a', 'source_b'):
        for T in (np.eye(4), R.T_STAR):
            idx, _, _ = R.nearest_within(R.transform(T, d[src]), d['target'], R.RADIUS)
            assert (idx >= 0).all()
        for radius in (0.02, 0.05, 0.1):
            _, d1, d2 = R.nearest_within(R.transform(R.T_STAR, d[src]), d['target'], radius)
            assert (~R.decided(d1, d2, radius)).mean() <= 0.01
    idx, _, _ = R.nearest_within(R.transform(R.T_STAR, d['source_b']), d['target'], R.RADIUS)
    assert np.array_equal(idx, d['subset'])


@pytest.mark.parametrize('method', ['point', 'plane'])
def test_restatement_recovers_the_pose_on_source_b(method):
    d = R.standard_inputs()
    out = R.icp(d['source_b'], d['target'], R.RADIUS, method=method, normal=d['normal'])
    rot, trans = R.pose_error(out['transformation'])
    print('restatement, source B, %s: %d iterations, rotation error %.3g deg, translation error %.3g' % (
        method, out['iterations'], np.degrees(rot), trans))
    assert out['converged'] and out['iterations'] <= 30 and out['fitness'] == 1.0
    # the source is T*^-1 of target points rounded to fp32 (half an ulp of 0.5 = 3e-8 per coordinate): the pose is determined to
    # well below that
    assert np.degrees(rot) < 1e-5 and trans < 1e-7


@pytest.mark.parametrize('method', ['point', 'plane'])
@pytest.mark.parametrize('src', ['source_a', 'source_b'])
def test_update_functions_reproduce_the_restatement_step(method, src):
    reg, d = _register(), R.standard_inputs()
    centre = R.bbox_centre(d['target'])
    t64, n64 = d['target'].astype(np.float64), d['normal'].astype(np.float64)
    hist = R.icp(d[src], d['target'], R.RADIUS, method=method, normal=d['normal'], max_iteration=3)['history']
    for T in hist[:3]:
        p = R.transform(T, d[src])
        idx, _, _ = R.nearest_within(p, d['target'], R.RADIUS)
        m = idx >= 0
        s = R.sums(method, p, d['target'], idx, centre, d['normal'])
        if method == 'point':
            want, got = R.point_step(p[m], t64[idx[m]]), reg.kabsch_step(s, centre)
        else:
            want, got = R.plane_step(p[m], t64[idx[m]], n64[idx[m]], centre), reg.plane_step(s, centre)
        assert np.abs(got - want).max() <= 1e-12
        fit, rmse = reg.fitness_rmse(s, len(p))
        assert fit == m.mean() and abs(rmse - np.sqrt(((p[m] - t64[idx[m]]) ** 2).sum() / m.sum())) <= 1e-15


def test_rodrigues_hand_cases():
    reg = _register()
    assert np.array_equal(reg.rodrigues([0.0, 0.0, 0.0]), np.eye(3))
    Rz = reg.rodrigues([0.0, 0.0, np.pi / 2])
    assert np.abs(Rz - np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])).max() < 1e-15
    for angle in (1e-9, 1e-5, 0.9e-4, 1.1e-4, 1.0, np.pi - 1e-9):
        w = angle * np.array([2.0, -1.0, 2.0]) / 3.0
        M = reg.rodrigues(w)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(M) - 1.0) < 1e-14
        assert np.abs(M @ w - w).max() < 1e-15 * max(angle, 1.0)          # the axis stays
        assert abs(np.arccos(np.clip((np.trace(M) - 1.0) / 2.0, -1.0, 1.0)) - angle) < 2e-8 or angle < 1e-7
        assert np.abs(M - R.Rotation.from_rotvec(w).as_matrix()).max() < 1e-14


def test_kabsch_hand_cases():
    reg = _register()
    rs = np.random.RandomState(0)
    P = rs.randn(50, 3)
    centre = np.array([0.3, -0.2, 0.1])

    def packed(p, q):
        s = np.zeros(R.FIELDS)
        s[R.COUNT] = len(p)
        s[R.D2] = ((p - q) ** 2).sum()
        s[R.PT_P:R.PT_P + 3] = (p - centre).sum(0)
        s[R.PT_Q:R.PT_Q + 3] = (q - centre).sum(0)
        s[R.PT_PQ:R.PT_PQ + 9] = ((p - centre).T @ (q - centre)).reshape(9)
        return s

    M = reg.kabsch_step(packed(P, P), centre)                              # zero rotation
    assert np.abs(M - np.eye(4)).max() < 1e-14
    for T in (R.rigid((1, 2, 3), 5.0, (0.02, -0.015, 0.01)), R.rigid((0, 1, 0), 180.0 - 1e-6, (1.0, 2.0, 3.0))):
        Q = P @ T[:3, :3].T + T[:3, 3]
        M = reg.kabsch_step(packed(P, Q), centre)
        assert np.abs(M - T).max() < 1e-12
    # coplanar input: the third singular value is zero and a reflection fits as well as a rotation -- the rotation must come back
    flat = P.copy()
    flat[:, 2] = 0.0
    T = R.rigid((1, 0, 0), 170.0, (0.0, 0.0, 0.5))
    M = reg.kabsch_step(packed(flat, flat @ T[:3, :3].T + T[:3, 3]), centre)
    assert abs(np.linalg.det(M[:3, :3]) - 1.0) < 1e-12 and np.abs(M - T).max() < 1e-12
    mirror = flat * np.array([1.0, 1.0, -1.0])                             # (the same points: z is zero)
    M = reg.kabsch_step(packed(flat, mirror), centre)
    assert abs(np.linalg.det(M[:3, :3]) - 1.0) < 1e-12
    assert reg.kabsch_step(packed(P[:2], P[:2]), centre) is None          # fewer than three pairs


def test_plane_step_degenerate_systems():
    reg = _register()
    s = np.zeros(R.FIELDS)
    assert reg.plane_step(s, np.zeros(3)) is None and reg.kabsch_step(s, np.zeros(3)) is None
    s[R.COUNT] = 100.0                                                     # a plane: only three of the six parameters are constrained
    p = np.random.RandomState(1).rand(100, 3) * [1.0, 1.0, 0.0]
    n = np.tile([0.0, 0.0, 1.0], (100, 1))
    t = R.terms('plane', p + [0.0, 0.0, 0.01], p.astype(np.float32), np.arange(100), np.zeros(3), n)
    assert reg.plane_step(t.sum(0), np.zeros(3)) is None
    s5 = R.terms('plane', p[:5], p[:5].astype(np.float32), np.arange(5), np.zeros(3), n[:5]).sum(0)
    assert reg.plane_step(s5, np.zeros(3)) is None


def test_init_validation():
    reg = _register()
    assert np.array_equal(reg.check_transformation(None), np.eye(4))
    assert np.array_equal(reg.check_transformation(R.T_STAR.tolist()), R.T_STAR)
    import torch
    assert np.array_equal(reg.check_transformation(torch.from_numpy(R.T_STAR).float()), R.T_STAR.astype(np.float32).astype(np.float64))
    bad = R.T_STAR.copy()
    bad[3, 3] = 2.0
    nan = R.T_STAR.copy()
    nan[0, 0] = np.nan
    for T in (np.eye(3), np.zeros((4, 4, 1)), bad, nan, 'pose', [[1, 2], [3]]):
        with pytest.raises(ValueError):
            reg.check_transformation(T)


def test_icp_c_abi_argument_errors_without_a_gpu():
    """Both entry points validate before any launch: error code + message on a machine without a GPU, never an abort.  The pointers
    are host buffers that are never dereferenced (every call ends at a check)."""
    from nksr_amd import _lib
    lib = _lib.lib
    null = C.c_void_p(0)
    buf = (C.c_double * 64)()
    at = C.cast(buf, C.c_void_p)

    def err():
        return lib.nksr_last_error().decode()

    def acc(n_ref=10, grid=at, hcap=8, cell=0.1, inv_cell=10.0, perm=at, normal=at, source=at, n_src=5, pose=at, centre=at, radius=0.05,
            method=0, corr=at, partials=at):
        return lib.nksr_icp_accumulate(grid, n_ref, grid, grid, grid, grid, hcap, cell, inv_cell, perm, normal, source, n_src, pose, centre,
                                       radius, method, corr, partials, null)

    assert acc(n_src=-1) != 0 and 'negative' in err()
    assert acc(n_ref=-1) != 0 and 'negative' in err()
    for r in (0.0, -1.0, float('inf'), float('nan')):
        assert acc(radius=r) != 0 and 'radius' in err()
    for m in (-1, 2):
        assert acc(method=m) != 0 and 'method' in err()
    assert acc(n_src=0, grid=null, corr=null, partials=null) == 0          # nothing to do: OK, nothing touched
    assert acc(grid=null) != 0 and 'NULL grid' in err()
    assert acc(hcap=12) != 0 and 'power of two' in err()
    assert acc(cell=0.04) != 0 and 'must be >= radius' in err()
    for name in ('perm', 'source', 'pose', 'centre'):
        assert acc(**{name: null}) != 0 and 'NULL perm / source' in err()
    assert acc(method=1, normal=null) != 0 and 'normals' in err()
    assert acc(corr=null) != 0 and 'output' in err()
    assert acc(partials=null) != 0 and 'output' in err()
    assert lib.nksr_icp_reduce(at, -1, at, null) != 0 and 'negative' in err()
    assert lib.nksr_icp_reduce(null, 4, at, null) != 0 and 'NULL' in err()
    assert lib.nksr_icp_reduce(at, 4, null, null) != 0 and 'NULL' in err()


def test_argument_checks_that_need_no_gpu():
    import torch
    reg = _register()
    src = torch.zeros((4, 3))
    with pytest.raises(ValueError):
        reg.icp(src, torch.zeros((0, 3)), 0.1)                                # empty target
    with pytest.raises(RuntimeError):
        reg.icp(src, torch.zeros((5, 3)), 0.1)                                # CPU tensors: the product path is GPU-only
    with pytest.raises(RuntimeError):
        reg.apply_transform(src, np.eye(4))
    with pytest.raises(ValueError):
        reg.apply_transform(src, np.eye(3))
    with pytest.raises(ValueError):
        reg.icp_multiscale(src, src, [0.1, 0.05], [0.2], [10, 10])
