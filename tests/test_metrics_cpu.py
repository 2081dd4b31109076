"""MeshEvaluator without a GPU: the C-ABI of the metric kernels rejects bad arguments before any launch, and the public surface
carries the reference's metric names and signatures."""
import ctypes as C
import inspect

import pytest


def _err():
    from nksr_amd import _lib
    return _lib.lib.nksr_last_error().decode()


def test_metric_entry_points_reject_bad_arguments():
    from nksr_amd import _lib
    lib = _lib.lib
    null = C.c_void_p(0)
    buf = (C.c_float * 64)()
    # face areas: negative sizes, faces over no vertices, NULL arrays
    assert lib.nksr_mesh_face_areas(buf, C.c_int64(-1), buf, 0, C.c_int64(1), buf, buf, null) != 0 and 'negative' in _err()
    assert lib.nksr_mesh_face_areas(buf, C.c_int64(3), buf, 0, C.c_int64(-2), buf, buf, null) != 0 and 'negative' in _err()
    assert lib.nksr_mesh_face_areas(buf, C.c_int64(0), buf, 0, C.c_int64(1), buf, buf, null) != 0 and 'zero vertices' in _err()
    assert lib.nksr_mesh_face_areas(null, C.c_int64(3), buf, 1, C.c_int64(1), buf, buf, null) != 0 and 'NULL' in _err()
    assert lib.nksr_mesh_face_areas(buf, C.c_int64(3), buf, 1, C.c_int64(1), buf, null, null) != 0 and 'NULL' in _err()
    # sampler: n_points > 0 with zero faces, negative sizes, NULL arrays
    assert lib.nksr_mesh_sample(buf, C.c_int64(3), buf, 0, C.c_int64(0), buf, buf, C.c_int64(10), C.c_uint64(0), buf, buf, buf, null) != 0
    assert 'zero faces' in _err()
    assert lib.nksr_mesh_sample(buf, C.c_int64(3), buf, 0, C.c_int64(1), buf, buf, C.c_int64(-5), C.c_uint64(0), buf, buf, buf, null) != 0
    assert 'negative' in _err()
    assert lib.nksr_mesh_sample(buf, C.c_int64(3), buf, 0, C.c_int64(1), null, buf, C.c_int64(5), C.c_uint64(0), buf, buf, buf, null) != 0
    assert 'NULL' in _err()
    assert lib.nksr_mesh_sample(buf, C.c_int64(3), buf, 0, C.c_int64(1), buf, buf, C.c_int64(5), C.c_uint64(0), buf, buf, null, null) != 0
    assert 'NULL' in _err()
    # the fp64 scan behind the CDF
    assert lib.nksr_inclusive_sum_f64(null, None, null, null, C.c_int64(10), null) != 0 and 'tmp_bytes' in _err()
    nbytes = C.c_size_t(0)
    assert lib.nksr_inclusive_sum_f64(null, C.byref(nbytes), null, null, C.c_int64(-1), null) != 0 and 'negative' in _err()
    # 1-NN with the metric epilogue
    pyr = _lib.KnnPyramidT()
    keys = (C.c_int64 * 4)()
    assert lib.nksr_nn_metrics(C.byref(pyr), keys, 1, null, buf, null, C.c_int64(-3), 4, buf, null, null, null) != 0 and 'negative' in _err()
    assert lib.nksr_nn_metrics(C.byref(pyr), keys, 1, null, null, null, C.c_int64(3), 4, buf, null, null, null) != 0 and 'NULL' in _err()
    assert lib.nksr_nn_metrics(C.byref(pyr), keys, 0, null, buf, null, C.c_int64(3), 4, buf, null, null, null) != 0 and 'empty' in _err()
    assert lib.nksr_nn_metrics(C.byref(pyr), keys, 1, null, buf, null, C.c_int64(3), 4, null, null, null, null) != 0 and 'no output' in _err()
    assert lib.nksr_nn_metrics(C.byref(pyr), keys, 1, null, buf, null, C.c_int64(3), 4, null, buf, null, null) != 0 and 'normal' in _err()
    assert lib.nksr_nn_metrics(None, keys, 1, null, buf, null, C.c_int64(3), 4, buf, null, null, null) != 0 and 'pyramid' in _err()
    assert lib.nksr_nn_metrics(C.byref(pyr), keys, 1, null, buf, null, C.c_int64(3), 4, buf, null, null, null) != 0 and 'pyramid' in _err()
    # the reduce
    assert lib.nksr_metric_reduce(null, C.c_int64(4), buf, null) != 0 and 'NULL' in _err()
    assert lib.nksr_metric_reduce(buf, C.c_int64(-4), buf, null) != 0 and 'negative' in _err()
    with pytest.raises(RuntimeError):
        _lib.call('nksr_metric_reduce', None, 4, None, None)


def test_metric_names_are_the_references():
    from nksr_amd.metrics import MeshEvaluator, THRESHOLDS
    assert MeshEvaluator.ESSENTIAL_METRICS == ['chamfer-L1', 'f-score', 'normals']
    assert MeshEvaluator.ALL_METRICS == ['completeness', 'accuracy', 'normals completeness', 'normals accuracy', 'normals', 'completeness2',
                                         'accuracy2', 'chamfer-L2', 'chamfer-L1', 'f-precision', 'f-recall', 'f-score', 'f-score-15',
                                         'f-score-20']
    assert THRESHOLDS == (0.01, 0.015, 0.02, 0.002, 0.1)


def test_metric_api_signatures():
    import nksr
    from nksr.metrics import MeshEvaluator, distance_p2p, sample_surface
    assert nksr.metrics.MeshEvaluator is MeshEvaluator
    sig = inspect.signature(MeshEvaluator.__init__)
    assert list(sig.parameters)[1:] == ['n_points', 'metric_names', 'device']
    assert sig.parameters['n_points'].default == 100000 and sig.parameters['metric_names'].default == MeshEvaluator.ALL_METRICS
    assert list(inspect.signature(MeshEvaluator.eval_mesh).parameters)[1:] == ['mesh', 'pointcloud_tgt', 'normals_tgt', 'onet_samples', 'seed']
    assert list(inspect.signature(MeshEvaluator.evaluate).parameters)[1:] == ['pointcloud', 'pointcloud_tgt', 'normals', 'normals_tgt']
    assert list(inspect.signature(distance_p2p).parameters)[:4] == ['src', 'nsrc', 'tgt', 'ntgt']
    assert list(inspect.signature(sample_surface).parameters)[:4] == ['v', 'f', 'n', 'seed']


def test_evaluator_refuses_the_cpu():
    from nksr_amd.metrics import MeshEvaluator
    with pytest.raises(RuntimeError):
        MeshEvaluator(device='cpu')
    with pytest.raises(RuntimeError):
        MeshEvaluator(1000, MeshEvaluator.ESSENTIAL_METRICS, device='cpu')
