"""nksr_amd/cloud_input.py, the input layer of the cloud tools, and what every public entry raises for a bad argument -- on a machine
without a GPU, so only the checks that come before the device is looked at, and the device check itself.  The table of exception
classes was taken from the modules as they were before they shared one input layer: callers tell RuntimeError from ValueError."""
import numpy as np
import pytest
import torch

nan, inf = float('nan'), float('inf')


class _NoIndex:
    """stands for a CloudIndex in the calls whose argument checks come before the index is used"""
    n, device = 10, torch.device('cpu')

    def __getattr__(self, name):
        raise AssertionError('the index was used (%s) before the arguments were checked' % name)


def _table():
    from nksr_amd import cloud
    x, nr = torch.zeros((10, 3)), torch.ones((10, 3))
    idx = torch.zeros((10, 2), dtype=torch.int32)
    feat = torch.zeros((10, 33))
    flat, two, ints, array = torch.zeros(10), torch.zeros((10, 2)), torch.zeros((10, 3), dtype=torch.int32), np.zeros((10, 3), np.float32)
    rows = []
    for name, bad in (('1-d', flat), ('[N,2]', two), ('integer', ints), ('numpy', array)):
        rows += [
            ('CloudIndex(%s)' % name, lambda bad=bad: cloud.CloudIndex(bad), RuntimeError),
            ('voxel_downsample(%s)' % name, lambda bad=bad: cloud.voxel_downsample(bad, 0.1), RuntimeError),
            ('statistical_outlier_mask(%s)' % name, lambda bad=bad: cloud.statistical_outlier_mask(bad), RuntimeError),
            ('orient_graph(xyz=%s)' % name, lambda bad=bad: cloud.orient_graph(bad, nr, idx), RuntimeError),
            ('orient_normals(xyz=%s)' % name, lambda bad=bad: cloud.orient_normals(bad, nr, k=2), RuntimeError),
            ('estimate_normals(%s)' % name, lambda bad=bad: cloud.estimate_normals(bad, knn=4, orient_k=2), RuntimeError),
            ('apply_transform(%s)' % name, lambda bad=bad: cloud.apply_transform(bad, np.eye(4)), RuntimeError),
            ('icp(target=%s)' % name, lambda bad=bad: cloud.icp(x, bad, 0.1), RuntimeError),
            ('cluster_dbscan(%s)' % name, lambda bad=bad: cloud.cluster_dbscan(bad, 0.1, 4), RuntimeError),
            ('sample_planes(%s)' % name, lambda bad=bad: cloud.sample_planes(bad, 8), RuntimeError),
            ('plane_scores(%s)' % name, lambda bad=bad: cloud.plane_scores(bad, np.zeros((2, 4)), 0.1), RuntimeError),
            ('segment_plane(%s)' % name, lambda bad=bad: cloud.segment_plane(bad, 0.1), RuntimeError),
            ('compute_fpfh_feature(xyz=%s)' % name, lambda bad=bad: cloud.compute_fpfh_feature(bad, nr, 0.1), RuntimeError),
            ('ransac(source=%s)' % name, lambda bad=bad: cloud.registration_ransac_based_on_feature_matching(bad, x, feat, feat, 0.1), RuntimeError),
            ('register_global(source=%s)' % name, lambda bad=bad: cloud.register_global(bad, x, 0.1), RuntimeError),
            ('mls_project(%s)' % name, lambda bad=bad: cloud.mls_project(bad, 0.1), RuntimeError),
            ('smooth_mls(%s)' % name, lambda bad=bad: cloud.smooth_mls(bad, 0.1), RuntimeError),
        ]
    for v in (0.0, -1.0, inf, nan):
        rows += [
            ('voxel_downsample(voxel_size=%r)' % v, lambda v=v: cloud.voxel_downsample(x, v), ValueError),
            ('radius_count(radius=%r)' % v, lambda v=v: cloud.CloudIndex.radius_count(_NoIndex(), v), ValueError),
            ('cluster_dbscan(eps=%r)' % v, lambda v=v: cloud.cluster_dbscan(x, v, 4), ValueError),
            ('CloudIndex.cluster_dbscan(eps=%r)' % v, lambda v=v: cloud.CloudIndex.cluster_dbscan(_NoIndex(), v, 4), ValueError),
            ('CloudIndex.compute_fpfh_feature(radius=%r)' % v, lambda v=v: cloud.CloudIndex.compute_fpfh_feature(_NoIndex(), nr, v), ValueError),
            ('ransac(max_correspondence_distance=%r)' % v,
             lambda v=v: cloud.registration_ransac_based_on_feature_matching(x, x, feat, feat, v), ValueError),
            ('register_global(voxel_size=%r)' % v, lambda v=v: cloud.register_global(x, x, v), ValueError),
            ('mls_project(radius=%r)' % v, lambda v=v: cloud.mls_project(x, v), ValueError),
            ('mls_project(sigma=%r)' % v, lambda v=v: cloud.mls_project(x, 0.1, sigma=v), ValueError),
            ('smooth_mls(radius=%r)' % v, lambda v=v: cloud.smooth_mls(x, v), ValueError),
            ('CloudIndex.mls_project(sigma=%r)' % v, lambda v=v: cloud.CloudIndex.mls_project(_NoIndex(), 0.1, sigma=v), ValueError),
        ]
    for name, bad in (('9 rows', torch.zeros((9, 3))), ('[N,2]', two), ('integer', ints), ('numpy', array)):
        rows += [
            ('mls_project(normal=%s)' % name, lambda bad=bad: cloud.mls_project(x, 0.1, normal=bad), ValueError),
            ('smooth_mls(normal=%s)' % name, lambda bad=bad: cloud.smooth_mls(x, 0.1, normal=bad), ValueError),
            ('CloudIndex.mls_project(normal=%s)' % name, lambda bad=bad: cloud.CloudIndex.mls_project(_NoIndex(), 0.1, normal=bad), ValueError),
            ('CloudIndex.compute_fpfh_feature(normal=%s)' % name,
             lambda bad=bad: cloud.CloudIndex.compute_fpfh_feature(_NoIndex(), bad, 0.1), RuntimeError),
        ]
    for name, bad in (('1-d', flat), ('[N,2]', two), ('integer', ints), ('numpy', array)):
        rows.append(('orient_graph(normal=%s)' % name, lambda bad=bad: cloud.orient_graph(x, bad, idx), RuntimeError))
    return rows


def test_every_bad_argument_raises_the_class_it_always_raised():
    rows = _table()
    assert len(rows) > 100
    for name, call, error in rows:
        with pytest.raises((RuntimeError, ValueError)) as e:
            call()
        assert type(e.value) is error, '%s raised %s (%s), not %s' % (name, type(e.value).__name__, e.value, error.__name__)


def test_every_public_entry_refuses_a_cpu_tensor():
    from nksr_amd import cloud
    x, nr = torch.zeros((10, 3)), torch.ones((10, 3))
    idx = torch.zeros((10, 2), dtype=torch.int32)
    feat = torch.zeros((10, 33))
    calls = {
        'CloudIndex': lambda: cloud.CloudIndex(x),
        'voxel_downsample': lambda: cloud.voxel_downsample(x, 0.1),
        'radius_outlier_mask': lambda: cloud.radius_outlier_mask(x, 0.1, 2),
        'statistical_outlier_mask': lambda: cloud.statistical_outlier_mask(x),
        'orient_graph': lambda: cloud.orient_graph(x, nr, idx),
        'orient_normals': lambda: cloud.orient_normals(x, nr, k=2),
        'estimate_normals': lambda: cloud.estimate_normals(x, knn=4, orient_k=2),
        'icp': lambda: cloud.icp(x, x, 0.1),
        'evaluate_registration': lambda: cloud.evaluate_registration(x, x, 0.1),
        'icp_multiscale': lambda: cloud.icp_multiscale(x, x, [0.1], [0.2], [3]),
        'apply_transform': lambda: cloud.apply_transform(x, np.eye(4)),
        'cluster_dbscan': lambda: cloud.cluster_dbscan(x, 0.1, 4),
        'sample_planes': lambda: cloud.sample_planes(x, 8),
        'plane_scores': lambda: cloud.plane_scores(x, np.zeros((2, 4)), 0.1),
        'segment_plane': lambda: cloud.segment_plane(x, 0.1),
        'compute_fpfh_feature': lambda: cloud.compute_fpfh_feature(x, nr, 0.1),
        'match_features': lambda: cloud.match_features(feat, feat),
        'registration_ransac_based_on_feature_matching': lambda: cloud.registration_ransac_based_on_feature_matching(x, x, feat, feat, 0.1),
        'register_global': lambda: cloud.register_global(x, x, 0.1),
        'mls_project': lambda: cloud.mls_project(x, 0.1),
        'smooth_mls': lambda: cloud.smooth_mls(x, 0.1),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match='GPU|cuda|MI355X'):
            call()


# ---- the layer itself --------------------------------------------------------------------------------------------------------------------
def test_positive():
    from nksr_amd import cloud_input as ci
    assert ci.positive(2, 'f', 'radius') == 2.0 and type(ci.positive(2, 'f', 'radius')) is float
    assert ci.positive(np.float32(0.5), 'f', 'radius') == 0.5 and ci.positive(True, 'f', 'radius') == 1.0
    assert ci.positive(5e-324, 'f', 'radius') == 5e-324
    for v in (0.0, -0.0, -1.0, inf, -inf, nan, False):
        with pytest.raises(ValueError, match='f: radius must be positive and finite'):
            ci.positive(v, 'f', 'radius')
    with pytest.raises(ValueError, match='^eps must be'):
        ci.positive(0, None, 'eps')
    for v in (None, 'x', [1.0, 2.0]):
        with pytest.raises((TypeError, ValueError)):
            ci.positive(v, 'f', 'radius')


def test_rows3_and_points_without_a_gpu():
    from nksr_amd import cloud_input as ci
    for good in (torch.zeros((0, 3)), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float16),
                 torch.zeros((6, 3))[::2]):
        ci.rows3(good, 'f')
        with pytest.raises(RuntimeError, match='GPU|cuda|MI355X'):        # the shape passes; the device does not
            ci.points(good, 'f')
    for bad in (torch.zeros(3), torch.zeros((4, 2)), torch.zeros((2, 4, 3)), torch.zeros((4, 3), dtype=torch.int64),
                torch.zeros((4, 3), dtype=torch.bool), np.zeros((4, 3), np.float32), [[0.0, 0.0, 0.0]], None):
        for check in (ci.rows3, ci.points):
            with pytest.raises(RuntimeError, match=r'f: query must be a floating-point \[N,3\] tensor'):
                check(bad, 'f', 'query')
    with pytest.raises(RuntimeError, match=r'^xyz must be'):
        ci.rows3(torch.zeros(3), None)


def test_all_finite():
    from nksr_amd import cloud_input as ci
    ci.all_finite(torch.zeros((0, 3)), 'f')
    ci.all_finite(torch.full((4, 3), 3e38), 'f')
    for v in (nan, inf, -inf):
        x = torch.zeros((4, 3))
        x[2, 1] = v
        with pytest.raises(RuntimeError, match='f: xyz: non-finite'):
            ci.all_finite(x, 'f')


def test_rows_like():
    from nksr_amd import cloud_input as ci
    cpu = torch.device('cpu')
    ci.rows_like(torch.zeros((4, 3)), 4, cpu, 'f', 'normal')
    ci.rows_like(torch.zeros((4, 3), dtype=torch.int32), 4, None, 'f', 'normal')         # any dtype unless floating is asked for
    ci.rows_like(torch.zeros((0, 3)), 0, None, 'f', 'normal', floating=True)
    for bad in (torch.zeros((3, 3)), torch.zeros((4, 2)), torch.zeros(4), torch.zeros((4, 3, 1)), np.zeros((4, 3)), None):
        with pytest.raises(RuntimeError, match=r'f: normal must be a \[4, 3\] tensor'):
            ci.rows_like(bad, 4, None, 'f', 'normal')
        with pytest.raises(ValueError, match='normal'):
            ci.rows_like(bad, 4, None, 'f', 'normal', error=ValueError)
    for bad in (torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 3), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='floating-point'):
            ci.rows_like(bad, 4, None, 'f', 'normal', floating=True)
    with pytest.raises(RuntimeError, match='normal is on cpu, the cloud on meta'):       # the device: a RuntimeError whatever `error` says
        ci.rows_like(torch.zeros((4, 3)), 4, torch.device('meta'), 'f', 'normal', error=ValueError)
