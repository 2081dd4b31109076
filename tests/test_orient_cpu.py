"""nksr_amd/orient.py without a GPU: the numpy reference (tests/orient_ref.py) on analytic shapes and hand-made graphs, the exported
names, the refusal of CPU tensors, the argument checks of the C entry points, and the header / bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cloud_ref
import orient_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('nksr_orient_init', 'nksr_orient_propose', 'nksr_orient_hook', 'nksr_orient_jump', 'nksr_orient_relabel', 'nksr_orient_seeds',
                'nksr_orient_apply')


def _random_flips(nrm, seed=3):
    sign = np.where(np.random.RandomState(seed).rand(len(nrm)) < 0.5, -1.0, 1.0).astype(np.float32)
    return nrm * sign[:, None]


def test_reference_orients_a_sphere_outward():
    from nksr_amd import utils
    xyz, nrm = utils.synth_sphere(2000, 0.45)
    idx, _ = cloud_ref.knn(xyz, 8, exclude_self=True)
    given = _random_flips(nrm)
    flipped, comp, ncomp = R.orient(xyz, given, idx[:, :8])
    out = R.apply(given, flipped)
    assert ncomp == 1 and (comp == 0).all()
    assert ((out * nrm).sum(1) > 0).all()
    assert 0.4 < flipped.mean() < 0.6
    # the viewpoint rule with the viewpoint at the centre turns the sphere inward
    flipped, _, _ = R.orient(xyz, given, idx[:, :8], viewpoint=(0.0, 0.0, 0.0))
    assert ((R.apply(given, flipped) * nrm).sum(1) < 0).all()


def test_reference_two_disjoint_spheres_are_two_components():
    from nksr_amd import utils
    a, na = utils.synth_sphere(1500, 0.2, 0.0, 0, center=(-0.3, 0.0, 0.0))
    b, nb = utils.synth_sphere(1500, 0.2, 0.0, 1, center=(0.3, 0.0, 0.0))
    xyz, nrm = np.concatenate([a, b]).astype(np.float32), np.concatenate([na, nb]).astype(np.float32)
    idx, _ = cloud_ref.knn(xyz, 8, exclude_self=True)
    given = _random_flips(nrm)
    flipped, comp, ncomp = R.orient(xyz, given, idx[:, :8])
    assert ncomp == 2 and (comp[:1500] == 0).all() and (comp[1500:] == 1).all()
    assert ((R.apply(given, flipped) * nrm).sum(1) > 0).all()


def test_reference_small_graphs():
    # a path 0 - 1 - 2 whose second edge flips; the seed is the highest point, 2, which looks down: it is flipped, and 1 and 0, which
    # disagree with it across the flipping edge, stay
    xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 1]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, -1]], np.float32)
    flipped, comp, ncomp = R.orient(xyz, nrm, np.array([[1], [2], [-1]]))
    assert ncomp == 1 and comp.tolist() == [0, 0, 0] and flipped.tolist() == [0, 0, 1]
    # the viewpoint below point 0 makes 0 the seed: it must look down
    flipped, _, _ = R.orient(xyz, nrm, np.array([[1], [2], [-1]]), viewpoint=(0.0, 0.0, -5.0))
    assert flipped.tolist() == [1, 1, 0]
    # ignored entries: self, negative, out of range; labels follow the minimum index; a zero normal flips nothing
    idx = np.array([[0, -1], [3, 3], [7, 2], [1, -5]])
    flipped, comp, ncomp = R.orient(np.zeros((4, 3), np.float32), np.array([[0, 0, 1], [0, 0, 0], [0, 0, -1], [0, 0, -1]], np.float32), idx)
    assert ncomp == 3 and comp.tolist() == [0, 1, 2, 1] and flipped.tolist() == [0, 0, 1, 0]
    # keys: weight bits above the slot, the weight clamped at 0
    key, u, v, flip = R.edge_keys(np.array([[0, 0, 2], [0, 0, -1]], np.float32), np.array([[1], [0]]))
    assert key.tolist() == [0, 1] and flip.tolist() == [True, True] and (u.tolist(), v.tolist()) == ([0, 1], [1, 0])
    key, _, _, _ = R.edge_keys(np.array([[0, 0, 1], [1, 0, 0]], np.float32), np.array([[1], [-1]]))
    assert key.tolist() == [0x3F800000 << 32]


def test_new_names_are_exported():
    import nksr
    assert 'get_estimate_oriented_normal_preprocess_fn' in nksr.__all__ and callable(nksr.get_estimate_oriented_normal_preprocess_fn())
    import nksr.cloud as cloud
    for name in ('orient_graph', 'orient_normals', 'estimate_normals', 'OrientedNormals'):
        assert callable(getattr(cloud, name)), name
    assert callable(cloud.CloudIndex.orient_normals)
    assert cloud.OrientedNormals._fields == ('normal', 'flipped', 'component', 'n_components')


def test_orient_refuses_cpu_tensors():
    import torch
    import nksr
    x, nr = torch.zeros((10, 3)), torch.ones((10, 3))
    idx = torch.zeros((10, 2), dtype=torch.int32)
    for call in (lambda: nksr.cloud.orient_graph(x, nr, idx), lambda: nksr.cloud.orient_normals(x, nr, k=2),
                 lambda: nksr.cloud.estimate_normals(x, knn=4, orient_k=2),
                 lambda: nksr.get_estimate_oriented_normal_preprocess_fn(4, 2)(x, None, None)):
        with pytest.raises(RuntimeError, match='MI355X'):
            call()


def test_orient_argument_errors():
    import torch
    import nksr
    x, nr = torch.zeros((10, 3)), torch.ones((10, 3))
    idx = torch.zeros((10, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match='seed'):
        nksr.cloud.orient_graph(x, nr, idx, seed='-z')
    with pytest.raises(ValueError, match='viewpoint'):
        nksr.cloud.orient_graph(x, nr, idx, viewpoint=(0.0, 1.0))
    with pytest.raises(ValueError, match='viewpoint'):
        nksr.cloud.orient_normals(x, nr, viewpoint=(0.0, float('nan'), 0.0))
    with pytest.raises(ValueError, match='seed'):
        nksr.cloud.estimate_normals(x, seed='up')
    with pytest.raises(RuntimeError, match='normal already exists'):
        nksr.get_estimate_oriented_normal_preprocess_fn()(x, nr, None)
    with pytest.raises(RuntimeError, match=r'\[N,3\]'):
        nksr.cloud.orient_graph(torch.zeros(10), nr, idx)
    # the sensor-based function is as it was
    with pytest.raises(RuntimeError, match='please provide sensor positions'):
        nksr.get_estimate_normal_preprocess_fn()(x, None, None)


def test_orient_c_abi_argument_errors_without_a_gpu():
    """Argument validation happens before any launch: error code + message on a machine without a GPU."""
    from nksr_amd import _lib
    lib = _lib.lib
    null = C.c_void_p(0)
    f = (C.c_float * 64)()
    i = (C.c_int32 * 64)()
    b = (C.c_uint8 * 64)()
    q = (C.c_uint64 * 64)()
    i64, ci, cf = C.c_int64, C.c_int, C.c_float

    def err():
        return lib.nksr_last_error().decode()

    def propose(n=4, k=2, normal=f, idx=i, rep=i, done=b, best=q, counters=i):
        return lib.nksr_orient_propose(normal, idx, i64(n), ci(k), null, rep, done, best, counters, null)
    assert propose(k=0) != 0 and '<= 32' in err()
    assert propose(k=_lib.ORIENT_MAX_K + 1) != 0 and '<= 32' in err()
    assert propose(n=-1) != 0 and '2^31' in err()
    assert propose(n=1 << 31) != 0 and '2^31' in err()
    assert propose(n=1 << 30, k=4) != 0 and '32 bits' in err()
    assert propose(idx=null) != 0 and 'NULL' in err()
    assert propose(counters=null) != 0 and 'NULL' in err()
    assert propose(n=0) == 0

    def hook(n=4, k=2, link=i, lpar=b):
        return lib.nksr_orient_hook(f, i, i64(n), ci(k), i, b, q, link, lpar, i, null)
    assert hook(k=33) != 0 and '<= 32' in err()
    assert hook(link=null) != 0 and 'NULL' in err()
    assert hook(n=0) == 0

    i2, b2 = (C.c_int32 * 64)(), (C.c_uint8 * 64)()
    assert lib.nksr_orient_jump(i, i64(4), i, b, i, b2, null) != 0 and 'different buffers' in err()
    assert lib.nksr_orient_jump(i, i64(4), i, b, i2, b, null) != 0 and 'different buffers' in err()
    assert lib.nksr_orient_jump(i, i64(4), i, b, null, b2, null) != 0 and 'NULL' in err()
    assert lib.nksr_orient_jump(i, i64(0), i, b, i2, b2, null) == 0
    assert lib.nksr_orient_init(i64(4), null, b, b, q, null) != 0 and 'NULL' in err()
    assert lib.nksr_orient_init(i64(0), null, null, null, null, null) == 0
    assert lib.nksr_orient_relabel(i64(4), i, b, null, b, q, null) != 0 and 'NULL' in err()
    assert lib.nksr_orient_relabel(i64(0), i, b, i, b, q, null) == 0

    def seeds(n=4, mode=0, v=(0.0, 0.0, 0.0), key=q):
        return lib.nksr_orient_seeds(f, i64(n), i, ci(mode), cf(v[0]), cf(v[1]), cf(v[2]), key, i, null)
    assert seeds(mode=2) != 0 and 'seed mode' in err()
    assert seeds(mode=_lib.ORIENT_SEED_VIEWPOINT, v=(0.0, float('inf'), 0.0)) != 0 and 'viewpoint' in err()
    assert seeds(key=null) != 0 and 'NULL' in err()
    assert seeds(n=0) == 0

    def apply(n=4, mode=0, flags=i, out=f):
        return lib.nksr_orient_apply(f, f, i64(n), i, b, q, i, ci(mode), cf(0), cf(0), cf(0), b, out, i, flags, null)
    assert apply(mode=-1) != 0 and 'seed mode' in err()
    assert apply(flags=null) != 0 and 'NULL' in err()
    assert apply(out=null) != 0 and 'NULL' in err()


def test_header_declares_and_lib_binds_the_orient_entry_points():
    from nksr_amd import _lib, build
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nksr_hip.h')).read(), flags=re.S)
    assert 'orient.hip' in build.SOURCES
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+%s\s*\(' % name, src), name
        assert name in _lib.EXPORTED and getattr(_lib.lib, name).argtypes is not None
    assert _lib.ORIENT_MAX_K == 32 and (_lib.ORIENT_SEED_Z, _lib.ORIENT_SEED_VIEWPOINT) == (0, 1)
