"""nksr_amd/mesh_input.py without a GPU: the recentring is a float64 difference rounded once, and the two face readers differ where
their callers need them to (numpy arrays and CPU tensors, dev = 'cpu')."""
import numpy as np
import pytest
import torch

OFFSET = np.array([1e7, -2e7, 3e7])


def _cloud():
    """Five points with features of size 1e-3 at OFFSET (float64), and a centre that float32 does not hold exactly."""
    rs = np.random.RandomState(3)
    return OFFSET + 1e-3 * rs.uniform(-1.0, 1.0, (5, 3)), OFFSET + np.array([0.3, -0.7, 1.1]) + 1e-3 / 3.0


def test_recentre_takes_the_difference_in_float64():
    from nksr_amd.mesh_input import recentre
    x64, centre = _cloud()
    out = recentre(x64, centre, 'cpu', 'x')
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (5, 3)
    assert np.array_equal(out.numpy(), np.float32(x64 - centre))
    assert not np.array_equal(out.numpy(), np.float32(x64) - np.float32(centre))
    assert np.array_equal(recentre(torch.from_numpy(x64), centre, 'cpu', 'x').numpy().view(np.uint32), out.numpy().view(np.uint32))


def test_recentre_refuses_bad_input():
    from nksr_amd.mesh_input import recentre
    x64, centre = _cloud()
    for bad in (np.nan, np.inf):
        x = x64.copy()
        x[2, 1] = bad
        with pytest.raises(ValueError, match='non-finite'):
            recentre(x, centre, 'cpu', 'x')
        with pytest.raises(ValueError, match='non-finite'):
            recentre(torch.from_numpy(x), centre, 'cpu', 'x')
    with pytest.raises(ValueError, match='queries'):
        recentre(x64[:, :2], centre, 'cpu', 'queries')
    assert tuple(recentre(np.zeros((0, 3)), centre, 'cpu', 'x').shape) == (0, 3)


def test_bbox_centre():
    from nksr_amd.mesh_input import bbox_centre
    x64, _ = _cloud()
    c = bbox_centre(x64)
    assert c.dtype == np.float64 and np.array_equal(c, 0.5 * (x64.min(0) + x64.max(0)))
    assert np.array_equal(bbox_centre(torch.from_numpy(x64)), c)
    x32 = x64.astype(np.float32)
    assert bbox_centre(x32).dtype == np.float64 and np.array_equal(bbox_centre(torch.from_numpy(x32)), bbox_centre(x32))
    for empty in (np.zeros((0, 3)), torch.zeros((0, 3))):
        with pytest.raises(ValueError, match='empty'):
            bbox_centre(empty)
    with pytest.raises(ValueError, match='target'):
        bbox_centre(np.zeros((4, 2)))


def _both(f, nv, **kw):
    from nksr_amd.mesh_input import faces
    a, b = faces(np.asarray(f), nv, 'cpu', **kw), faces(torch.from_numpy(np.asarray(f)), nv, 'cpu', **kw)
    assert a.dtype == b.dtype and torch.equal(a, b) and a.is_contiguous()
    return a


EVALUATOR = dict(cast_float=True, check_range=True)         # MeshEvaluator, MeshQuery, sample_surface
TOPOLOGY = dict(cast_float=False, check_range=False)        # MeshTopology
TRI = [[0, 1, 2], [2, 1, 3]]


@pytest.mark.parametrize('mode', [EVALUATOR, TOPOLOGY], ids=['evaluator', 'topology'])
def test_faces_common_to_both_readers(mode):
    from nksr_amd.mesh_input import faces, is64
    for dt, want in ((np.int32, torch.int32), (np.int64, torch.int64), (np.int16, torch.int64), (np.uint8, torch.int64)):
        t = _both(np.array(TRI, dt), 4, **mode)
        assert t.dtype == want and t.tolist() == TRI and is64(t) == int(want == torch.int64)
    for empty in (np.zeros((0, 3), np.int32), np.zeros(0, np.int16), torch.zeros(0, dtype=torch.int64)):
        assert tuple(faces(empty, 4, 'cpu', **mode).shape) == (0, 3)
    assert tuple(faces([], 4, 'cpu', **EVALUATOR).shape) == (0, 3)          # ([] is a float64 array: the topology reader refuses it)
    assert faces(np.zeros((0, 3), np.int32), 4, 'cpu', **mode).dtype == torch.int32
    with pytest.raises(ValueError, match='faces'):
        _both(np.zeros((2, 4), np.int64), 4, **mode)
    with pytest.raises(ValueError, match='faces'):
        _both(np.zeros(6, np.int64), 4, **mode)


def test_faces_float_and_bool_indices():
    as_stored = np.array(TRI, np.float64)           # bench.py keeps mesh_faces.npy in floating point
    t = _both(as_stored, 4, **EVALUATOR)
    assert t.dtype == torch.int64 and t.tolist() == TRI
    assert _both(as_stored.astype(np.float32), 4, **EVALUATOR).dtype == torch.int64
    for bad in (as_stored, as_stored.astype(np.float32), np.array(TRI) > 0):
        with pytest.raises(ValueError, match='expected integer indices'):
            _both(bad, 4, **TOPOLOGY)
    with pytest.raises(ValueError, match='expected integer indices'):
        _both(np.zeros((0, 3), np.float32), 4, **TOPOLOGY)


@pytest.mark.parametrize('bad', [4, -1])
@pytest.mark.parametrize('dt', [np.int32, np.int64])
def test_faces_out_of_range_indices(bad, dt):
    f = np.array(TRI, dt)
    f[1, 2] = bad
    with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
        _both(f, 4, **EVALUATOR)
    assert _both(f, 4, **TOPOLOGY).tolist() == f.tolist()       # MeshTopology counts it as an invalid face
    assert _both(np.array(TRI, dt), 4, **EVALUATOR).tolist() == TRI


def test_normals32():
    from nksr_amd.mesh_input import normals32
    n = np.random.RandomState(0).normal(size=(5, 3))
    assert normals32(None, 5, 'cpu', 'n') is None
    t = normals32(n, 5, 'cpu', 'n')
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), n.astype(np.float32))
    assert torch.equal(normals32(torch.from_numpy(n), 5, 'cpu', 'n'), t)
    with pytest.raises(ValueError, match='5 rows for 6 points'):
        normals32(n, 6, 'cpu', 'n')
    with pytest.raises(ValueError, match='normals_tgt'):
        normals32(n[:, :2], 5, 'cpu', 'normals_tgt')
    n[3, 0] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        normals32(n, 5, 'cpu', 'n')


def test_gpu_device_refuses_the_cpu():
    from nksr_amd.mesh_input import gpu_device
    with pytest.raises(RuntimeError):
        gpu_device('cpu')
    with pytest.raises(RuntimeError):
        gpu_device(torch.device('cpu'), like=torch.zeros(3))


def test_the_mesh_modules_share_one_input_layer():
    """mesh_input stands below the three mesh modules, and none of them keeps a helper of its own."""
    import nksr_amd.mesh_input as mi
    from nksr_amd import mesh_query, mesh_topology, metrics
    assert not {'metrics', 'mesh_query', 'mesh_topology', 'cloud'} & set(vars(mi))
    assert metrics.MeshQuery is mesh_query.MeshQuery and metrics.MeshTopology is mesh_topology.MeshTopology
    assert metrics.mesh_occupancy is mesh_query.mesh_occupancy
    for mod in (metrics, mesh_query, mesh_topology):
        assert not {'_bbox_centre', '_recentre', '_rows3', '_faces', '_normals32', '_device', '_is64'} & set(vars(mod)), mod.__name__
