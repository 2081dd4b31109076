"""nksr_amd/cloud.py without a GPU: the numpy / scipy reference (tests/cloud_ref.py) on hand-made cases, the argument checks of the
new C entry points, and the exported names."""
import ctypes as C

import numpy as np
import pytest

import cloud_ref as R


def test_reference_knn_on_a_line():
    x = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]], np.float64)
    j, d = R.knn(x, 2)
    assert j[:, :2].tolist() == [[0, 1], [1, 0], [2, 1], [3, 2]] and d[:, :3].tolist() == [[0, 1, 3], [0, 1, 2], [0, 2, 3], [0, 4, 6]]
    j, d = R.knn(x, 2, exclude_self=True)
    assert j[:, :2].tolist() == [[1, 2], [0, 2], [1, 0], [2, 1]] and d[:, :2].tolist() == [[1, 3], [1, 2], [2, 3], [4, 6]]
    j, d = R.knn(x, 1, query=np.array([[2.4, 0, 0]]))
    assert j[0, 0] == 2 and abs(d[0, 0] - 0.6) < 1e-15 and abs(d[0, 1] - 1.4) < 1e-15


def test_reference_knn_keeps_duplicates_of_the_query_point():
    x = np.concatenate([np.zeros((5, 3)), np.array([[1.0, 0, 0], [2.0, 0, 0]])])
    j, d = R.knn(x, 3, exclude_self=True)
    for i in range(5):                           # three of the four other copies, never the point itself
        assert i not in j[i, :3] and (d[i, :3] == 0).all() and set(j[i, :3]) <= set(range(5))
    assert d[5, :3].tolist() == [1, 1, 1]


def test_reference_radius_count_and_band():
    x = np.array([[0, 0, 0], [0.5, 0, 0], [1.0, 0, 0], [1.0 + 5e-6, 0, 0], [4, 0, 0]], np.float64)
    cnt, sure = R.radius_count(x, 0.75)
    assert cnt.tolist() == [2, 4, 3, 3, 1] and sure.all()
    cnt, sure = R.radius_count(x, 0.75, exclude_self=True)
    assert cnt.tolist() == [1, 3, 2, 2, 0]
    cnt, sure = R.radius_count(x, 1.0, query=np.array([[0.0, 0, 0], [3.5, 0, 0]]))
    assert cnt.tolist() == [3, 1] and sure.tolist() == [False, True]          # a point sits 5e-6 behind the radius of the first


def test_reference_statistical_outlier():
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.rand(200, 3), [[9.0, 9.0, 9.0]]])
    mask, m, thr = R.statistical_outlier(x, k=4, std_ratio=2.0)
    assert not mask[200] and mask[:200].mean() > 0.9
    _, d = R.knn(x, 4, exclude_self=True)
    assert np.allclose(m, d[:, :4].mean(1)) and abs(thr - (m.mean() + 2.0 * np.sqrt(((m - m.mean()) ** 2).sum() / 200))) < 1e-12


def test_reference_voxel_downsample():
    x = np.array([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [-0.1, 0.1, 0.1], [0.4, 0.2, 0.6], [1.0, 0.0, 0.0], [-1e-9, -1e-9, -1e-9]], np.float32)
    a = np.arange(12, dtype=np.float64).reshape(6, 2)
    r = R.voxel_downsample(x, 1.0, [a])
    # floor puts -0.1 and -1e-9 into cell -1; ascending Morton order of the biased coordinates: z is the highest bit
    assert r['ijk'].tolist() == [[-1, -1, -1], [-1, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert r['inverse'].tolist() == [2, 2, 1, 2, 3, 0] and r['count'].tolist() == [1, 1, 3, 1] and r['first'].tolist() == [5, 2, 0, 4]
    assert np.allclose(r['xyz'][2], x[[0, 1, 3]].astype(np.float64).mean(0)) and np.allclose(r['attrs'][0][2], a[[0, 1, 3]].mean(0))
    # the voxel is decided in float32: 0.3 / 0.1 is 3.0000001 there (2.9999999... in float64)
    assert R.voxel_ijk(np.array([[0.3, 0.3, 0.3]], np.float32), 0.1).tolist() == [[3, 3, 3]]
    n = R.unit_normals(np.array([[0, 0, 2.0], [0, 0, 0]]), np.array([[1.0, 0, 0], [0, 1.0, 0]]))
    assert n.tolist() == [[0, 0, 1], [0, 1, 0]]


def test_new_names_are_exported():
    import nksr
    for name in ('get_voxel_downsample_preprocess_fn', 'get_radius_outlier_preprocess_fn', 'get_statistical_outlier_preprocess_fn',
                 'compose_preprocess_fns', 'cloud'):
        assert name in nksr.__all__ and hasattr(nksr, name)
    import nksr.cloud as cloud
    for name in ('CloudIndex', 'voxel_downsample', 'radius_outlier_mask', 'statistical_outlier_mask'):
        assert callable(getattr(cloud, name))
    seen = []
    fn = nksr.compose_preprocess_fns(lambda x, n, s: (seen.append(1) or x + 1, n, s), lambda x, n, s: (seen.append(2) or x * 2, n, s))
    assert fn(1, None, 'sensor') == (4, None, 'sensor') and seen == [1, 2]


def test_cloud_refuses_cpu_tensors():
    import torch
    import nksr
    x = torch.zeros((10, 3))
    for call in (lambda: nksr.cloud.CloudIndex(x), lambda: nksr.cloud.voxel_downsample(x, 0.1),
                 lambda: nksr.cloud.radius_outlier_mask(x, 0.1, 2), lambda: nksr.cloud.statistical_outlier_mask(x, 4)):
        with pytest.raises(RuntimeError):
            call()


def test_cloud_c_abi_argument_errors_without_a_gpu():
    """Argument validation happens before any launch: error code + message on a machine without a GPU."""
    from nksr_amd import _lib
    lib = _lib.lib
    null = C.c_void_p(0)
    one = (C.c_float * 64)()
    ints = (C.c_int32 * 64)()
    longs = (C.c_int64 * 64)()

    def err():
        return lib.nksr_last_error().decode()

    i64, i32, ci, cf = C.c_int64, C.c_int32, C.c_int, C.c_float
    grid = (ints, ints, longs, ints, i32(8), cf(1.0), cf(1.0))

    pyr = _lib.KnnPyramidT()                  # one level, complete: the checks on the other arguments are reached
    pyr.xyz_sorted = C.cast(one, C.c_void_p)
    pyr.start[0], pyr.end[0], pyr.hvals[0] = (C.cast(ints, C.c_void_p),) * 3
    pyr.hkeys[0], pyr.hcap[0], pyr.levels, pyr.cell, pyr.inv_cell = C.cast(longs, C.c_void_p), 8, 1, 1.0, 1.0

    def knn_pyr(p=pyr, n_ref=10, query=one, nq=1, k=4, ex=0, rings=4, idx=ints, d2=one, valid=ints):
        return lib.nksr_knn_query_pyramid(C.byref(p) if p is not None else None, i64(n_ref), query, i64(nq), ci(k), ci(ex), null, ci(rings), idx,
                                          d2, valid, null)
    assert knn_pyr(k=33) != 0 and '<= 32' in err()
    assert knn_pyr(k=40) != 0 and '<= 32' in err()
    assert knn_pyr(k=0) != 0 and '<= 32' in err()
    assert knn_pyr(k=10, ex=1) != 0 and 'reference points' in err()
    assert knn_pyr(k=32, ex=1, n_ref=32) != 0 and 'reference points' in err()
    assert knn_pyr(nq=-1) != 0 and 'negative' in err()
    assert knn_pyr(rings=0) != 0 and 'max_ring' in err()
    assert knn_pyr(idx=null) != 0 and 'NULL' in err()
    assert knn_pyr(valid=null) != 0 and 'NULL' in err()
    assert knn_pyr(query=null, nq=11) != 0 and 'n_ref' in err()
    assert knn_pyr(p=_lib.KnnPyramidT()) != 0 and 'pyramid' in err()                 # levels = 0
    assert knn_pyr(p=None) != 0 and 'pyramid' in err()
    assert knn_pyr(nq=0) == 0

    def count(xyz=one, g=grid, query=one, nq=1, n_ref=10, radius=0.5, out=ints):
        return lib.nksr_radius_count(xyz, i64(n_ref), *g, query, i64(nq), cf(radius), i32(0), ci(0), null, out, null)
    assert count(radius=0.0) != 0 and 'radius' in err()
    assert count(radius=float('nan')) != 0 and 'radius' in err()
    assert count(radius=2.0) != 0 and '>= radius' in err()      # the grid's cell is 1
    assert count(out=null) != 0 and 'NULL' in err()
    assert count(xyz=null) != 0 and 'NULL' in err()
    assert count(g=(ints, ints, longs, ints, i32(12), cf(1.0), cf(1.0))) != 0 and 'power of two' in err()
    assert count(g=(ints, ints, longs, ints, i32(8), cf(0.0), cf(1.0))) != 0 and 'cell' in err()
    assert count(query=null, nq=11) != 0 and 'n_ref' in err()
    assert count(nq=0) == 0

    def reduce(order=ints, n=10, nvox=2, xyz=one, attr=null, c=0, group=0, mean=one, amean=null, cnt=ints):
        return lib.nksr_voxel_reduce(order, i64(n), ints, ints, i64(nvox), xyz, attr, ci(c), ci(group), mean, amean, cnt, null, null)
    assert reduce(order=null) != 0 and 'NULL' in err()
    assert reduce(mean=null) != 0 and 'NULL' in err()
    assert reduce(c=3) != 0 and 'attribute' in err()
    assert reduce(c=_lib.VOXEL_REDUCE_MAX_C + 1, attr=one, amean=one) != 0 and 'channels' in err()
    assert reduce(group=65) != 0 and 'group' in err()
    assert reduce(n=1, nvox=2) != 0 and 'n_vox' in err()
    assert reduce(n=-1) != 0 and 'n_vox' in err()
    assert reduce(n=1 << 31, nvox=1) != 0 and '2^31' in err()
    assert reduce(n=0, nvox=0) == 0
