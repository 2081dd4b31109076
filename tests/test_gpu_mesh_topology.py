"""Mesh topology on the MI355X (nksr_amd/mesh_topology.py, csrc/meshtopo.hip) against the numpy / scipy restatement
(tests/mesh_topology_ref.py).  Every comparison is exact except the fp64 component areas (relative 1e-12: the same fp64 face areas
summed in another order)."""
import numpy as np
import pytest
import torch

import mesh_topology_ref as T

pytestmark = pytest.mark.gpu

TOTALS = ('num_edges', 'boundary_edges', 'nonmanifold_edges', 'misoriented_edges', 'invalid_faces', 'referenced_vertices')
EDGE_ARRAYS = ('edges', 'edge_counts', 'edge_classes', 'face_adjacency')
LABELS = ('face_label', 'vertex_label')
COUNTS = ('face_count', 'vertex_count', 'edge_count', 'boundary_edges', 'euler', 'closed')
AREA_RTOL = 1e-12


def _topo(v, f):
    from nksr_amd.mesh_topology import MeshTopology
    return MeshTopology(v, f)


def _np(x):
    return x.cpu().numpy()


def _check_table(t, v, f):
    ref = T.edge_table(f, len(v))
    for k in TOTALS:
        assert getattr(t, k) == ref[k], (k, getattr(t, k), ref[k])
    assert t.euler_characteristic == ref['euler']
    for k in EDGE_ARRAYS:
        got = _np(getattr(t, k))
        assert got.shape == ref[k].shape and np.array_equal(got, ref[k]), k
    return ref


def _check_components(t, v, f, conn, stats=True):
    c, ref = t.components(conn), T.components(v, f, conn)
    assert c.n == ref['n']
    for k in LABELS:
        assert np.array_equal(_np(getattr(c, k)), ref[k]), (conn, k)
    if stats:
        for k in COUNTS:
            assert np.array_equal(_np(getattr(c, k)), ref[k]), (conn, k)
        assert np.array_equal(_np(c.box), ref['box']), conn
        area = _np(c.area)
        print(conn, 'max relative area error', float(np.max(np.abs(area - ref['area']) / np.maximum(ref['area'], 1e-300), initial=0.0)))
        assert np.all(np.abs(area - ref['area']) <= AREA_RTOL * ref['area'])
    return c, ref


def _check_all(v, f):
    t = _topo(v, f)
    _check_table(t, v, f)
    for conn in ('edge', 'vertex'):
        _check_components(t, v, f, conn)
    return t


# ---- hand-known meshes -----------------------------------------------------------------------------------------------------------
def test_sphere_torus_and_hollow_shell():
    v, f = T.uv_sphere(64, 32)
    t = _check_all(v, f)
    assert (t.boundary_edges, t.nonmanifold_edges, t.misoriented_edges) == (0, 0, 0) and t.euler_characteristic == 2
    assert t.is_closed and t.is_edge_manifold and t.is_oriented and t.is_watertight
    c = t.components()
    assert c.n == 1 and _np(c.euler).tolist() == [2] and _np(c.closed).tolist() == [True]
    assert t.components() is c and t.components('vertex') is not c
    v, f = T.torus(96, 48)
    t = _check_all(v, f)
    assert t.euler_characteristic == 0 and t.is_watertight and t.components().n == 1
    v, f = T.voxel_mesh(T.voxel_sets()['shell'], 0)
    t = _check_all(v, f)
    for conn in ('edge', 'vertex'):
        c = t.components(conn)
        assert c.n == 2 and _np(c.euler).tolist() == [2, 2] and _np(c.closed).tolist() == [True, True]
        assert _np(c.area).tolist() == [150.0, 42.0]
    assert t.is_watertight


def test_flipped_face_and_holes():
    v, f = T.uv_sphere(64, 32)
    g = f.copy()
    g[777] = g[777][::-1]
    t = _check_all(v, g)
    assert t.misoriented_edges == 3 and not t.is_oriented and not t.is_watertight and t.is_closed
    h = np.delete(f, np.random.RandomState(0).choice(len(f), 10, replace=False), 0)
    t = _check_all(v, h)
    assert t.boundary_edges == T.edge_table(h, len(v))['boundary_edges'] > 0 and not t.is_closed


def test_nonmanifold_fan_and_cubes_touching_at_a_vertex():
    v, f = T.three_fan()
    t = _check_all(v, f)
    assert t.nonmanifold_edges == 1 and not t.is_edge_manifold
    e = int(np.nonzero(_np(t.edge_classes) == T.NONMANIFOLD)[0][0])
    assert _np(t.edge_counts)[e] == 3 and _np(t.edges)[e].tolist() == [0, 1]
    assert (_np(t.face_adjacency) == -1).all() and t.components('edge').n == 1
    v, f = T.two_cubes_sharing_a_vertex()
    t = _check_all(v, f)
    assert t.components('vertex').n == 1 and t.components('edge').n == 2
    c = t.components('edge')
    assert _np(c.vertex_count).tolist() == [8, 8] and _np(c.euler).tolist() == [2, 2]


def test_invalid_faces_and_face_dtypes():
    v, f = T.uv_sphere(64, 32)
    bad = np.array([[5, 5, 9], [1, 2, len(v)], [3, -1, 4], [7, 8, 7], [0, 1, 1 << 40]], np.int64)
    at = [0, 100, 100, 2000, len(f)]
    g = np.insert(f, at, bad, 0)
    t = _check_all(v, g)
    s = _topo(v, f)
    assert t.invalid_faces == 5
    for k in TOTALS:
        if k != 'invalid_faces':
            assert getattr(t, k) == getattr(s, k), k
    assert t.euler_characteristic == 2 and np.array_equal(_np(t.edges), _np(s.edges))
    is_bad = ~T.valid_faces(g, len(v))
    assert is_bad.sum() == 5
    for conn in ('edge', 'vertex'):
        lab = _np(t.components(conn).face_label)
        assert (lab[is_bad] == -1).all() and (lab[~is_bad] == 0).all()
    assert (_np(t.face_adjacency)[is_bad] == -1).all()
    # int32 faces: the same results, array by array
    g32 = np.where(np.abs(g) < (1 << 31), g, -7).astype(np.int32)
    u = _topo(v, torch.from_numpy(g32))
    for k in TOTALS:
        assert getattr(t, k) == getattr(u, k), k
    for k in EDGE_ARRAYS:
        assert torch.equal(getattr(t, k), getattr(u, k)), k
    for conn in ('edge', 'vertex'):
        a, b = t.components(conn), u.components(conn)
        for k in LABELS + COUNTS + ('area', 'box'):
            assert torch.equal(getattr(a, k), getattr(b, k)), (conn, k)
    keep = np.ones(len(g), bool)
    f64, f32 = t.compact(keep)[1], u.compact(keep)[1]
    assert f64.dtype == torch.int64 and f32.dtype == torch.int32 and torch.equal(f64, f32.long()) and np.array_equal(_np(f64), f)


def test_empty_mesh_and_single_triangle():
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32))):
        t = _check_all(v, f)
        assert t.num_edges == 0 and t.euler_characteristic == 0 and t.is_closed and t.components().n == 0
        v2, f2, c2, vmap = t.compact(np.zeros(0, bool))
        assert v2.shape == (0, 3) and f2.shape == (0, 3) and c2 is None and _np(vmap).tolist() == [-1] * len(v)
        assert _np(t.components().select(min_faces=3)).shape == (0,)
    v = np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 2, 0]], np.float32)
    t = _check_all(v, np.array([[3, 0, 2]], np.int64))
    assert (t.num_edges, t.boundary_edges, t.referenced_vertices, t.euler_characteristic) == (3, 3, 3, 1)
    c = t.components()
    assert c.n == 1 and _np(c.vertex_label).tolist() == [0, -1, 0, 0] and _np(c.area).tolist() == [1.0]
    assert _np(c.box).tolist() == [[0, 0, 0, 1, 2, 0]]
    v2, f2, _, vmap = t.compact([True])
    assert _np(f2).tolist() == [[2, 0, 1]] and _np(vmap).tolist() == [0, -1, 1, 2] and np.array_equal(_np(v2), v[[0, 2, 3]])


def test_errors_are_exceptions():
    v, f = T.three_fan()
    t = _topo(v, f)
    with pytest.raises(ValueError):
        t.components('face')
    with pytest.raises(ValueError):
        t.compact(np.ones(2, bool))
    with pytest.raises(ValueError):
        t.components().select(min_area_ratio=2.0)
    with pytest.raises(ValueError):
        _topo(v, f.astype(np.float32))
    with pytest.raises(ValueError):
        _topo(v[:, :2], f)
    from nksr_amd.mesh_topology import MeshTopology
    with pytest.raises(RuntimeError):
        MeshTopology(v, f, device='cpu')


# ---- union-find worst cases (vertex and face order shuffled, fixed seed) ------------------------------------------------------------
@pytest.fixture(scope='module')
def soup():
    return T.shuffled(*T.random_soup(100000, 20000), seed=13)


@pytest.mark.parametrize('case', ['strip', 'disjoint', 'soup', 'dense_soup'])
def test_union_find_labels_equal_the_restatement(case, soup):
    if case == 'strip':         # one path of 200 000 faces: deep chains, contended hooks
        v, f = T.shuffled(*T.triangle_strip(200000), seed=11)
    elif case == 'disjoint':    # 50 000 roots
        v, f = T.shuffled(*T.disjoint_triangles(50000), seed=12)
    elif case == 'soup':        # 100 000 random faces over 20 000 vertices
        v, f = soup
    else:                       # 300 vertices only: ~7 faces round every edge, a third of the faces invalid or repeated
        v, f = T.shuffled(*T.random_soup(100000, 300, seed=6), seed=14)
    t = _topo(v, f)
    _check_table(t, v, f)
    n = {}
    for conn in ('edge', 'vertex'):
        n[conn] = _check_components(t, v, f, conn)[0].n
    if case == 'strip':
        assert n == {'edge': 1, 'vertex': 1}
    if case == 'disjoint':
        assert n == {'edge': 50000, 'vertex': 50000}


def test_two_builds_are_bitwise_equal(soup):
    v, f = soup
    a, b = _topo(v, f), _topo(v, f)
    for k in EDGE_ARRAYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert all(getattr(a, k) == getattr(b, k) for k in TOTALS)
    for conn in ('edge', 'vertex'):
        ca, cb = a.components(conn), b.components(conn)
        assert ca.n == cb.n
        for k in LABELS + COUNTS + ('box',):
            assert torch.equal(getattr(ca, k), getattr(cb, k)), (conn, k)
        assert torch.equal(ca.area.view(torch.int64), cb.area.view(torch.int64)), conn
    keep = torch.from_numpy(np.random.RandomState(1).rand(len(f)) < 0.5)
    for x, y in zip(a.compact(keep, v), b.compact(keep, v)):
        assert torch.equal(x, y)


# ---- cleanup -----------------------------------------------------------------------------------------------------------------------
def test_floaters_are_removed_and_keep_all_changes_nothing():
    from nksr_amd.fields.base_field import MeshingResult
    v, f, col, n0 = T.sphere_with_floaters(20)
    sv, sf = T.uv_sphere(64, 32)
    dev = torch.device('cuda:0')
    mesh = MeshingResult(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(col).to(dev))
    t = mesh.topology()
    assert t.components().n == 21 and _np(t.components().face_count).tolist() == [n0] + [4] * 20
    keep = np.arange(len(f)) < n0
    rv, rf, rc, rmap = T.compact(v, f, keep, col)
    assert np.array_equal(rv, sv) and np.array_equal(rf, sf)
    for kw in ({'min_faces': 10}, {'keep_largest': 1}, {'min_area_ratio': 0.01}, {'min_faces': 10, 'connectivity': 'vertex'}):
        out = mesh.remove_small_components(**kw)
        assert isinstance(out, MeshingResult) and out.f.dtype == mesh.f.dtype and out.v.dtype == mesh.v.dtype
        assert np.array_equal(_np(out.v), rv) and np.array_equal(_np(out.f), rf) and np.array_equal(_np(out.c), rc), kw
    assert np.array_equal(_np(t.compact(keep)[3]), rmap)
    area = T.components(v, f)['area']
    top3 = np.lexsort((np.arange(21), -area))[:3]                          # by area, then the lower id
    assert sorted(np.nonzero(_np(t.components().select(keep_largest=3)))[0].tolist()) == sorted(top3.tolist())
    assert _np(t.components().select(keep_largest=0)).sum() == 0
    # keep-all on a mesh without unreferenced vertices: v and f come back bit for bit (float64 vertices stay float64)
    for vv in (sv, sv.astype(np.float64) * (1 + 1e-12)):
        s = _topo(vv, sf)
        v2, f2, c2, vmap = s.compact(np.ones(len(sf), bool))
        assert v2.dtype == torch.from_numpy(vv).dtype and np.array_equal(_np(v2).view(np.uint8), vv.view(np.uint8)) and np.array_equal(_np(f2), sf)
        assert c2 is None and np.array_equal(_np(vmap), np.arange(len(sv)))
        v3, f3, _, _ = s.remove_small_components()
        assert torch.equal(v3, v2) and torch.equal(f3, f2)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_recipe_mesh_topology_and_cleanup():
    import nksr
    from conftest import make_cloud
    dev = torch.device('cuda:0')
    xyz, nrm = make_cloud('sphere', 3000, 0.005, 0)
    rec = nksr.Reconstructor(dev, config='snet-n3k-wnormal')
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=None)
    mesh = fld.extract_dual_mesh(mise_iter=1)
    v, f = _np(mesh.v), _np(mesh.f)
    t = mesh.topology()
    ref = _check_table(t, v, f)
    print('recipe mesh: faces', len(f), {k: ref[k] for k in TOTALS}, 'components', t.components().n)
    for conn in ('edge', 'vertex'):
        _check_components(t, v, f, conn)
    out = mesh.remove_small_components(min_area_ratio=0.01)
    assert out.f.shape[0] > 0 and int(out.f.min()) >= 0 and int(out.f.max()) < out.v.shape[0]
    c0, c1 = t.components(), out.topology().components()
    assert c1.n == int(c0.select(min_area_ratio=0.01).sum()) >= 1
    assert bool((c1.area >= 0.01 * c1.area.max()).all()) and float(c1.area.max()) == float(c0.area.max())
    assert out.topology().referenced_vertices == out.v.shape[0]
