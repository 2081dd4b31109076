"""Mesh cross-sections on the MI355X (nksr_amd/mesh_slice.py, csrc/meshslice.hip) against the numpy restatement (tests/mesh_slice_ref.py),
which is given the heights the GPU reports.  Every integer array is compared index for index, nothing left out and nothing masked; the
heights, points, lengths and areas within the bounds stated at ``check``.  Every comparison prints its largest error before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_slice_ref as R
import mesh_topology_ref as T

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
FLOATS = ('vertex_height', 'points64', 'polyline_length', 'polyline_area', 'plane_length', 'plane_area')


def _slicer(v, f):
    from nksr_amd.mesh_slice import MeshSlicer
    return MeshSlicer(v, f)


def _np(x):
    return x.cpu().numpy()


def _tensors(r):
    return {k: x for k, x in vars(r).items() if isinstance(x, torch.Tensor)}


def _same_bits(a, b):
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb) and set(FLOATS) | set(R.INTEGER_ARRAYS) <= set(ta)
    for k in ta:
        x, y = ta[k], tb[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


def check(v, f, normal, offsets, label, watertight=False, convex=False, slicer=None):
    """One slice against the restatement.  Bounds:
      heights   |h - numpy| <= 3 eps sum |n_i x_i|: two fused and one plain rounding against three products and two sums
      points    |p - ref| <= 4 eps (|a| + |b|) per component (the formula with or without contraction differs by one rounding of t (b - a))
      sums      |sum - math.fsum(terms)| <= n eps sum |term| over the n terms of a polyline or of a plane; the terms are the
                restatement's, evaluated at the points the GPU reports (which the line above has compared with its own)."""
    s = slicer or _slicer(v, f)
    r = s.slice(normal, offsets)
    n = np.array(r.normal)
    assert np.array_equal(n, R.unit(normal))
    x = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    h = _np(r.vertex_height)
    x64 = x.astype(np.float64)
    assert r.vertex_height.dtype == torch.float64 and h.shape == (len(x),)
    if len(x):
        err = np.abs(h - R.heights(x, n))
        bound = 3 * EPS * (np.abs(x64) * np.abs(n)).sum(1)
        print('%s: heights max err %.3g (bound %.3g)' % (label, err.max(), bound.max()))
        assert np.all(err <= bound)
    want = own = R.slice_mesh(x, f, n, offsets, h, points=_np(r.points64))        # ('points64' of the result stays the restatement's own)
    print('%s: N=%d S=%d L=%d P=%d' % (label, r.n_points, r.n_segments, r.n_polylines, r.n_planes))
    assert (r.n_points, r.n_segments, r.n_polylines) == (want['n_points'], want['n_segments'], want['n_polylines'])
    for k in R.INTEGER_ARRAYS:
        got = _np(getattr(r, k))
        assert got.shape == want[k].shape, (label, k, got.shape, want[k].shape)
        assert np.array_equal(got, want[k]), (label, k)
        if k not in ('point_start', 'seg_start', 'polyline_closed'):
            assert got.dtype == np.int32, (label, k, got.dtype)
    assert r.polyline_closed.dtype == torch.bool
    e = T.edge_table(f, len(x))['edges'][want['point_edge']].astype(np.int64).reshape(-1, 2)
    perr = np.abs(_np(r.points64) - own['points64'])
    pbound = 4 * EPS * (np.abs(x64[e[:, 0]]) + np.abs(x64[e[:, 1]]))
    print('%s: points max err %.3g (bound %.3g)' % (label, perr.max(initial=0.0), pbound.max(initial=0.0)))
    assert np.all(perr <= pbound)
    assert r.points.dtype == (torch.float64 if x.dtype == np.float64 else torch.float32) and torch.equal(r.points, r.points64.to(r.points.dtype))
    for name, terms in (('length', want['length_terms']), ('area', want['area_terms'])):
        got = _np(getattr(r, 'polyline_' + name))
        ref = np.array([math.fsum(t) for t in terms])
        bound = np.array([len(t) * EPS * math.fsum(abs(y) for y in t) for t in terms])
        err = np.abs(got - ref)
        print('%s: polyline %s max err %.3g (bound there %.3g)' % (label, name, err.max(initial=0.0), bound[np.argmax(err)] if len(err) else 0.0))
        assert np.all(err <= bound), (label, name)
        got = _np(getattr(r, 'plane_' + name))
        for j in range(r.n_planes):
            t = [y for l in range(want['plane_polyline_start'][j], want['plane_polyline_start'][j + 1]) for y in terms[l]]
            assert abs(got[j] - math.fsum(t)) <= len(t) * EPS * math.fsum(abs(y) for y in t), (label, name, j)
    assert not _np(r.polyline_area)[~want['polyline_closed']].any()
    for j in range(r.n_planes):
        a = r.polylines_of(j)
        assert (a.start, a.stop) == tuple(want['plane_polyline_start'][j:j + 2])
    if watertight:
        assert s.topology.is_watertight and want['polyline_closed'].all() and not want['plane_open'].any()
        for c in (0, 1):
            assert np.array_equal(np.sort(want['segments'][:, c]), np.arange(r.n_points))          # every point is tail once and head once
    if convex:
        assert np.all(_np(r.polyline_area)[_np(r.polyline_length) > 0] > 0)
    return r, want


@functools.lru_cache(maxsize=None)
def big_sphere():
    return R.icosphere(5)


def test_tetrahedron_planes_miss_cut_and_pass_through_vertices():
    v, f = R.tetrahedron()
    r, w = check(v, f, (0, 0, 1), [-1.0, 0.0, 0.5, 1.0, 2.0], 'tetra z', watertight=True, convex=True)
    assert list(w['polyline_plane']) == [2, 3] and _np(r.polyline_area)[0] == 0.125         # z = 0: the face in the plane is all above
    n = R.unit((1, 1, 0))
    h = R.heights(v, n)
    r, w = check(v, f, (1, 1, 0), [h[1]], 'tetra edge in the plane', watertight=True)
    assert _np(r.vertex_height)[1] == _np(r.vertex_height)[2] == h[1] and r.n_segments == 4 and _np(r.polyline_area)[0] == 0.0
    check(v, f, (1, 1, 1), [0.0, 0.25, 1.0 / math.sqrt(3.0)], 'tetra oblique', watertight=True, convex=True)


def test_cube_planes_at_the_vertex_heights_and_no_planes():
    v, f = R.cube((0, 0, 0), (2, 3, 1))
    r, w = check(v, f, (0, 0, 1), [0.0, 1.0], 'cube', watertight=True, convex=True)
    assert list(w['polyline_plane']) == [1] and list(_np(r.polyline_area)) == [6.0] and list(_np(r.polyline_length)) == [10.0]
    assert list(_np(r.plane_area)) == [0.0, 6.0]
    r, _ = check(v, f, (0, 0, 1), [], 'cube, no planes', watertight=True)
    assert r.n_points == r.n_segments == r.n_polylines == 0 and r.plane_area.shape == (0,) and r.polyline_start.tolist() == [0]


def test_empty_meshes():
    for v, f in ((np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64))):
        r, _ = check(v, f, (0, 1, 0), [-1.0, 0.0, 1.0], 'F = 0')
        assert r.n_segments == 0 and _np(r.plane_length).tolist() == [0.0] * 3 and _np(r.plane_open).tolist() == [0] * 3


def test_open_strip_gives_open_chains():
    v, f = R.strip(40, 7)
    r, w = check(v, f, (1, 0, 0), [0.5, 1.5, 2.0, 39.75, 41.0], 'strip')
    assert _np(r.plane_open).tolist() == [1, 1, 1, 1, 0] and not w['polyline_closed'].any() and list(_np(r.polyline_length)) == [7.0] * 4
    r, w = check(v, f, (1, 3, 0), np.linspace(0.0, 20.0, 33), 'strip oblique')
    assert _np(r.plane_open).sum() > 20


def test_flipped_face_and_nonmanifold_edge_end_chains():
    v, f = R.icosphere(1)
    g = f.copy()
    g[7] = g[7][[0, 2, 1]]
    r, w = check(v, g, (0, 0, 1), np.linspace(-0.9, 0.9, 7), 'flipped face')
    whole = R.slice_mesh(v, f, np.array(r.normal), np.linspace(-0.9, 0.9, 7), _np(r.vertex_height))
    assert r.n_segments == whole['n_segments'] and r.n_polylines > whole['n_polylines'] and _np(r.plane_open).any()
    v, f = T.three_fan()
    r, w = check(v, f, (1, 0, 0), [0.25, 0.5], 'three fan')
    assert r.n_segments == 6 and r.n_polylines == 6 and (w['succ'] == -1).all()


@pytest.mark.parametrize('fdt', [np.int32, np.int64])
@pytest.mark.parametrize('far', [False, True])
def test_several_loops_per_plane_and_their_signs(fdt, far):
    a, b = R.icosphere(2, 0.5), R.icosphere(2, 0.4)
    tv, tf = R.torus(48, 24, 2.75, 0.5)
    v, f = R.merged((a[0] + [0.0, 0.0, 0.1], a[1]), (b[0] + [0.0, 1.5, 0.0], b[1]), (tv, tf))
    v = v + 1e6 if far else v.astype(np.float32)
    offs = np.array([-0.3, 0.0, 0.1, 0.45]) + (1e6 if far else 0.0)
    r, w = check(v, f.astype(fdt), (0, 0, 1), offs, 'spheres and torus far=%s' % far, watertight=True)
    area = _np(r.polyline_area)
    for j in range(4):
        a = area[r.polylines_of(j)]
        assert len(a) == (4 if j < 3 else 3) and (a < 0).sum() == 1 and (a > 0).sum() == len(a) - 1       # one hole: the torus' inner loop
    assert r.points.dtype == (torch.float64 if far else torch.float32)


def test_invalid_faces_cross_nothing():
    v, f = R.cube()
    g = np.concatenate([f[:5], [[0, 99, 3], [-1, 2, 3]], f[5:], [[4, 4, 7]]])
    r, w = check(v, g, (0, 0, 1), [0.25, 0.5], 'invalid faces')
    assert not np.isin(w['segment_face'], [5, 6, len(g) - 1]).any() and r.n_segments == 16 and w['polyline_closed'].all()


def test_oblique_normal_on_dyadic_coordinates_with_planes_through_vertices():
    v, f = R.merged(R.cube((0, 0, 0), (1, 2, 1)), (R.tetrahedron()[0] + [4.0, 0.0, 0.0], R.tetrahedron()[1]), R.strip(3, 2))
    s = _slicer(v.astype(np.float32), f)
    h = np.unique(_np(s.slice((1, 1, 1), []).vertex_height))
    assert len(h) < len(v)                                  # several vertices share a height
    r, w = check(v.astype(np.float32), f, (1, 1, 1), h, 'dyadic oblique', slicer=s)
    assert r.n_segments > 20


def test_oblique_normal_on_random_coordinates():
    v, f = R.icosphere(3)
    rs = np.random.RandomState(5)
    v = v * rs.uniform(0.7, 1.3, (len(v), 1)) + rs.normal(size=(1, 3)) * 10
    check(v, f, rs.normal(size=3), np.sort(rs.uniform(-15, 15, 40)), 'random oblique fp64', watertight=True)
    check(v.astype(np.float32), f, (0.3, -2.0, 0.9), np.sort(rs.uniform(-15, 15, 40)), 'random oblique fp32', watertight=True)


def test_thousand_levels_and_determinism():
    v, f = R.icosphere(3)
    levels = np.linspace(-1.1, 1.1, 1000)
    r, w = check(v.astype(np.float32), f, (0, 0, 1), levels, '1000 levels', watertight=True, convex=True)
    assert r.n_planes == 1000 and r.n_polylines > 800 and _np(r.plane_open).sum() == 0
    s = _slicer(v.astype(np.float32), f)
    _same_bits(r, s.slice((0, 0, 1), levels))
    # the points kernel's other shape (one lane per edge, or one per point): the same three arrays
    from nksr_amd import mesh_slice
    lo_f, seg_start, lo_e, point_start = mesh_slice.plane_ranges(r.vertex_height, s.f, s.topology.face_valid, s.topology.edges, r.offsets)
    for by_point in (0, 1):
        got = mesh_slice.edge_points(s.x, r.vertex_height, s.topology.edges, r.offsets, lo_e, point_start, r.n_points, by_point=by_point)
        assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
                   for a, b in zip(got, (r.points64, r.point_edge, r.point_plane)))
    # more planes than the LDS stage holds: the same answer through the other counting kernel
    v, f = R.icosphere(1)
    check(v.astype(np.float32), f, (0, 0, 1), np.linspace(-1.1, 1.1, 3001), '3001 levels', watertight=True)


def test_long_loops_with_the_smallest_id_in_the_middle():
    v, f = R.cylinder(3000, 2)
    s = _slicer(v, f)
    r, w = check(v, f, (0, 0, 1), [0.5, 1.0, 1.5], 'cylinder', slicer=s)
    assert r.n_polylines == 3 and w['polyline_closed'].all() and np.diff(w['polyline_start']).tolist() == [6000] * 3
    assert r.rounds == math.ceil(math.log2(r.n_segments)) + 1 == 16
    rank_of_neighbour = w['segment_rank'][w['succ'][w['polyline_rep']]]
    assert (rank_of_neighbour == 1).all() and (w['segment_rank'][w['pred'][w['polyline_rep']]] == 5999).all()
    first = np.nonzero(w['segment_plane'] == 0)[0]
    assert w['polyline_rep'][0] == first.min() and abs(int(w['segment_face'][first.min()]) - int(w['segment_face'][w['pred'][first.min()]])) > 1000
    area = math.pi                                                       # the 3000-gon: pi (1 - O(1e-6))
    assert np.all(np.abs(_np(r.polyline_area) - area) < 1e-5) and np.all(np.abs(_np(r.polyline_length) - 2 * math.pi) < 1e-5)
    _same_bits(r, s.slice((0, 0, 1), [0.5, 1.0, 1.5]))
    _same_bits(r, _slicer(v, f).slice((0, 0, 2.5), [0.5, 1.0, 1.5]))


def test_sphere_section_areas_within_the_chord_error():
    """The mesh lies between the spheres of radius r and sqrt(r^2 - e^2 / 3) (e: its longest edge; no point of a triangle with corners
    on the sphere and sides <= e is further in), and it is star-shaped about the centre, so the section at offset o lies between the
    discs of radius^2 r^2 - o^2 and r^2 - e^2 / 3 - o^2:  0 <= pi (r^2 - o^2) - area <= pi e^2 / 3."""
    v, f = big_sphere()
    assert len(f) == 20480
    e = np.linalg.norm(v[f] - v[np.roll(f, -1, 1)], axis=2).max()
    offs = np.array([-0.9, -0.5, 0.0, 0.3, 0.7, 0.95])
    r, w = check(v, f, (0, 0, 1), offs, 'sphere 20480', watertight=True, convex=True)
    exact = math.pi * (1.0 - offs ** 2)
    got = _np(r.plane_area)
    print('sphere: exact - area', exact - got, 'allowed', math.pi * e * e / 3)
    assert np.all(exact - got >= -1e-12) and np.all(exact - got <= math.pi * e * e / 3 + 1e-12)
    assert np.all(np.abs(got - w['plane_area']) <= 1e-12) and r.n_polylines == 6


def test_other_entrances_give_the_same_tensors(tmp_path):
    import nksr
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_slice import MeshSlicer
    from nksr_amd.mesh_topology import MeshTopology
    v, f = R.torus(48, 24, 2.75, 0.5)
    levels = [-0.25, 0.0, 0.25]
    direct = MeshSlicer(v, f).slice((0, 0, 1), levels)
    topo = MeshTopology(v, f)
    _same_bits(direct, MeshSlicer.from_topology(topo).slice((0, 0, 1), levels))
    mesh = MeshingResult(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda())
    _same_bits(direct, mesh.contours(levels=levels))
    _same_bits(direct, mesh.slice((0, 0, 3), levels))
    by_interval = MeshSlicer(v, f).contours(interval=0.125)
    z = v[:, 2].astype(np.float64)
    multiples = [k * 0.125 for k in range(-8, 9) if z.min() < k * 0.125 <= z.max()]        # the multiples in (min z, max z]
    assert _np(by_interval.offsets).tolist() == multiples and 6 <= len(multiples) <= 8
    _same_bits(by_interval, MeshSlicer(v, f).slice((0, 0, 1), multiples))
    _same_bits(MeshSlicer(v, f).contours(levels=[2.5], axis=0), MeshSlicer(v, f).slice((1, 0, 0), [2.5]))
    with pytest.raises(TypeError):
        MeshSlicer.from_topology(mesh)
    path = str(tmp_path / 'contours.obj')
    nksr.utils.write_obj_polylines(path, direct.points64, direct.polyline_start, direct.polyline_points)
    vs = np.array([[float(x) for x in l.split()[1:]] for l in open(path) if l.startswith('v ')])
    ls = [[int(x) - 1 for x in l.split()[1:]] for l in open(path) if l.startswith('l ')]
    assert np.array_equal(vs, _np(direct.points64)) and len(ls) == direct.n_polylines == 6
    start, ids = _np(direct.polyline_start), _np(direct.polyline_points)
    assert all(ls[k] == ids[start[k]:start[k + 1]].tolist() for k in range(6))


def test_argument_errors_are_value_errors():
    v, f = R.tetrahedron()
    s = _slicer(v, f)
    for normal in ((0, 0, 0), (0.0, float('nan'), 1.0), (1, 2), 'up'):
        with pytest.raises(ValueError):
            s.slice(normal, [0.5])
    for offsets in ([0.5, 0.25], [0.5, 0.5], [0.0, float('inf')], [float('nan')], [[0.1, 0.2]], 'abc'):
        with pytest.raises(ValueError):
            s.slice((0, 0, 1), offsets)
    with pytest.raises(ValueError):
        _slicer(v, f.astype(np.float32))
    for kw in ({}, {'levels': [0.5], 'interval': 0.1}, {'interval': 0.0}, {'interval': float('nan')}, {'levels': [0.5], 'axis': 3}):
        with pytest.raises(ValueError):
            s.contours(**kw)
    assert s.slice((0, 0, 1), torch.tensor([0.5])).n_segments == 3        # and the slicer still works
