"""Mesh clipping on the MI355X (nksr_amd/mesh_clip.py, csrc/meshclip.hip) against the numpy restatement (tests/mesh_clip_ref.py), which
is given the heights and the points the GPU reports.  Every integer array is compared index for index, nothing left out and nothing
masked; the cut points bit for bit with the slicer's; the attributes and the areas within the bounds stated at ``check`` and at
``mesh_clip_ref.area_bound``.  Every comparison prints its largest error before it asserts."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_clip_ref as R
import mesh_topology_ref as T

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_TENSORS = R.INTEGER_ARRAYS + ('v2_64', 'vertex_height', 'offsets')


def _clipper(v, f, attr=None):
    from nksr_amd.mesh_clip import MeshClipper
    return MeshClipper(v, f, attr)


def _np(x):
    return x.cpu().numpy()


def _tensors(r):
    return {k: x for k, x in vars(r).items() if isinstance(x, torch.Tensor)}


def _bits(x):
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else (x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x)


def _same_bits(a, b, need=SPLIT_TENSORS):
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb) and set(need) <= set(ta), (sorted(ta), sorted(tb))
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape, k
        assert torch.equal(_bits(ta[k]), _bits(tb[k])), k


def _same_mesh(a, b):
    """Two MeshingResults (or (v, f, c) tuples of numpy arrays) with equal bits."""
    for name in ('v', 'f', 'c'):
        x, y = (getattr(m, name) if hasattr(m, name) else m['vfc'.index(name)] for m in (a, b))
        assert (x is None) == (y is None), name
        if x is not None:
            x, y = (_np(t) if isinstance(t, torch.Tensor) else np.asarray(t) for t in (x, y))
            assert x.dtype == y.dtype and x.shape == y.shape, (name, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name


def check(v, f, normal, offsets, label, attr=None, clipper=None):
    """One split against the restatement.
      integers  every array of INTEGER_ARRAYS index for index, with its dtype; the counts
      vertices  v2_64[:V] is the input widened exactly; v2_64[V:] equals MeshSlicer.slice(...).points64 bit for bit
      attr      |attr2 - ref| <= 4 eps (|a| + |b|) per channel at the points (the slicer's point bound: the formula with or without
                contraction differs by one rounding of t (b - a)); the vertex rows are the input widened exactly"""
    from nksr_amd.mesh_slice import MeshSlicer
    c = clipper or _clipper(v, f, attr)
    r = c.split(normal, offsets)
    n = np.array(r.normal)
    assert np.array_equal(n, R.unit(normal))
    x = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    nv = len(x)
    h = _np(r.vertex_height)
    want = R.split_mesh(x, f, n, offsets, h, points=_np(r.v2_64[nv:]), attr=attr)
    print('%s: V=%d N=%d F2=%d parts=%d dropped=%d degenerate=%d' % (label, nv, r.n_points, r.n_faces, r.n_parts, r.n_dropped, r.n_degenerate))
    got_counts = (r.n_vertices, r.n_points, r.n_faces, r.n_parts, r.n_dropped, r.n_degenerate)
    assert got_counts == (nv, want['n_points'], want['n_faces'], want['n_parts'], want['n_dropped'], want['n_degenerate']), (label, got_counts)
    for k in R.INTEGER_ARRAYS:
        got = _np(getattr(r, k))
        assert got.shape == want[k].shape, (label, k, got.shape, want[k].shape)
        assert got.dtype == (np.int64 if k in ('face_start', 'point_start') else np.int32), (label, k, got.dtype)
        assert np.array_equal(got, want[k]), (label, k)
    assert r.v2_64.dtype == torch.float64 and np.array_equal(_np(r.v2_64[:nv]).view(np.int64), x.astype(np.float64).view(np.int64))
    s = MeshSlicer.from_topology(c.topology).slice(normal, offsets)
    assert torch.equal(r.v2_64[nv:].contiguous().view(torch.int64), s.points64.view(torch.int64)), label
    assert torch.equal(r.vertex_height.view(torch.int64), s.vertex_height.view(torch.int64))
    for k in ('point_edge', 'point_plane', 'point_start'):
        assert torch.equal(getattr(r, k), getattr(s, k)), k
    perr = np.abs(_np(r.v2_64[nv:]) - want['points64'])                    # (the restatement's own points: the slicer's bound)
    e = T.edge_table(f, nv)['edges'][want['point_edge']].astype(np.int64).reshape(-1, 2)
    x64 = x.astype(np.float64)
    pbound = 4 * EPS * (np.abs(x64[e[:, 0]]) + np.abs(x64[e[:, 1]]))
    print('%s: points max err %.3g (bound %.3g)' % (label, perr.max(initial=0.0), pbound.max(initial=0.0)))
    assert np.all(perr <= pbound)
    vdt = torch.float64 if x.dtype == np.float64 else torch.float32
    assert r.v2.dtype == vdt and torch.equal(r.v2, r.v2_64.to(vdt)) and r.f2.shape == (r.n_faces, 3)
    if attr is None:
        assert r.attr2 is None and r.attr2_64 is None
    else:
        a64 = np.asarray(attr).astype(np.float64)
        got = _np(r.attr2_64)
        assert r.attr2_64.dtype == torch.float64 and got.shape == (nv + r.n_points, a64.shape[1])
        assert np.array_equal(got[:nv].view(np.int64), a64.view(np.int64))
        aerr = np.abs(got[nv:] - want['attr2_64'][nv:])
        abound = 4 * EPS * (np.abs(a64[e[:, 0]]) + np.abs(a64[e[:, 1]]))
        print('%s: attr max err %.3g (bound %.3g)' % (label, aerr.max(initial=0.0), abound.max(initial=0.0)))
        assert np.all(aerr <= abound)
        adt = torch.float64 if np.asarray(attr).dtype == np.float64 else torch.float32
        assert r.attr2.dtype == adt and torch.equal(r.attr2, r.attr2_64.to(adt))
    # both shapes of the face kernel, and a second call: equal tensors bit for bit
    for by_piece in (0, 1):
        _same_bits(r, c.split(normal, offsets, _by_piece=by_piece))
    return r, want


def check_parts(r, want, label, labels=None, n_labels=None):
    """``parts`` against the restatement's grouping, and every part's mesh against the restatement's."""
    p = r.parts() if labels is None else r.parts(labels, n_labels)
    k = r.n_parts if labels is None else n_labels
    g = R.group(want['f2'], want['face_part'] if labels is None else labels, k)
    for name in R.GROUP_ARRAYS:
        got = _np(getattr(p, name))
        assert got.dtype == g[name].dtype and got.shape == g[name].shape, (label, name, got.dtype, got.shape, g[name].shape)
        assert np.array_equal(got, g[name]), (label, name)
    assert len(p) == k and p.nonempty == [j for j in range(k) if g['part_face_start'][j + 1] > g['part_face_start'][j]]
    v2, c2 = _np(r.v2), None if r.attr2 is None else _np(r.attr2)
    for j in range(k):
        _same_mesh(p[j], R.part_mesh(g, j, v2, c2))
    assert len(list(p)) == len(p.nonempty)
    return p, g


@functools.lru_cache(maxsize=None)
def big_sphere():
    return R.icosphere(5)


def _colors(v, channels=3, dtype=np.float32, seed=0):
    return np.random.default_rng(seed).uniform(-1, 2, (len(v), channels)).astype(dtype)


def test_tetrahedron_planes_miss_cut_and_pass_through_a_vertex_an_edge_and_a_face():
    v, f = R.tetrahedron()
    r, w = check(v, f, (0, 0, 1), [-1.0, 0.0, 0.5, 1.0, 2.0], 'tetra z', attr=_colors(v))
    assert set(w['face_part']) == {2, 3, 4} and r.n_degenerate == 6
    check_parts(r, w, 'tetra z')
    n = R.unit((1, 1, 0))
    r, w = check(v, f, (1, 1, 0), [R.heights(v, n)[1]], 'tetra edge in the plane')
    assert r.n_points == 4 and r.n_faces == 12 and r.n_degenerate == 8
    check(v, f, (1, 1, 1), [0.0, 0.25, 1.0 / math.sqrt(3.0)], 'tetra oblique', attr=_colors(v, 5, np.float64))
    r, _ = check(v, f, (0, 0, 1), [5.0, 6.0], 'tetra missed')
    assert r.n_points == 0 and r.n_faces == 4 and _np(r.face_part).tolist() == [0] * 4


def test_cube_planes_at_the_vertex_heights_and_no_planes():
    v, f = R.cube((0, 0, 0), (2, 3, 1))
    r, w = check(v, f, (0, 0, 1), [0.0, 1.0], 'cube', attr=_colors(v, 1))
    assert r.n_points == 8 and r.n_faces == 28 and r.n_degenerate == 16
    r, _ = check(v, f, (0, 0, 1), [], 'cube, no planes', attr=_colors(v, 4))
    assert r.n_points == 0 and r.n_parts == 1 and torch.equal(r.f2.cpu(), torch.from_numpy(f).to(torch.int32))
    assert torch.equal(r.face_source.cpu(), torch.arange(12, dtype=torch.int32)) and r.attr2.shape == (8, 4)
    r, w = check(v, f, (0, 0, 1), [0.5], 'cube z = 0.5')
    p, _ = check_parts(r, w, 'cube z = 0.5')
    assert [float(R.face_areas(_np(m.v), _np(m.f))[0].sum()) for m in p] == [6.0 + 5.0, 6.0 + 5.0]


def test_empty_meshes():
    for v, f in ((np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64))):
        r, w = check(v, f, (0, 1, 0), [-1.0, 0.0, 1.0], 'F = 0', attr=_colors(v, 2))
        assert r.n_faces == 0 and r.n_points == 0 and r.n_parts == 4 and r.f2.shape == (0, 3)
        p, _ = check_parts(r, w, 'F = 0')
        assert p.nonempty == [] and p[2].v.shape == (0, 3) and p[2].f.shape == (0, 3)


def test_open_strip():
    v, f = R.strip(40, 7)
    r, w = check(v, f, (1, 0, 0), [0.5, 1.5, 2.0, 39.75, 41.0], 'strip', attr=_colors(v))
    check_parts(r, w, 'strip')
    check(v, f, (1, 3, 0), np.linspace(0.0, 20.0, 33), 'strip oblique')


def test_flipped_face_and_nonmanifold_edge():
    v, f = R.icosphere(1)
    g = f.copy()
    g[7] = g[7][[0, 2, 1]]
    check(v, g, (0, 0, 1), np.linspace(-0.9, 0.9, 7), 'flipped face')
    v, f = T.three_fan()
    r, _ = check(v, f, (1, 0, 0), [0.25, 0.5], 'three fan')
    assert r.n_faces == 3 * 5


def test_invalid_faces_are_dropped_and_counted():
    v, f = R.cube()
    g = np.concatenate([f[:5], [[0, 99, 3], [-1, 2, 3]], f[5:], [[4, 4, 7]]])
    r, w = check(v, g, (0, 0, 1), [0.25, 0.5], 'invalid faces', attr=_colors(v))
    assert r.n_dropped == 3 and not np.isin(w['face_source'], [5, 6, len(g) - 1]).any() and r.n_faces == 4 + 8 * 5


@pytest.mark.parametrize('fdt', [np.int32, np.int64])
@pytest.mark.parametrize('far', [False, True])
def test_spheres_and_torus_dtypes_and_far_coordinates(fdt, far):
    a, b = R.icosphere(2, 0.5), R.icosphere(2, 0.4)
    tv, tf = R.torus(48, 24, 2.75, 0.5)
    v, f = R.merged((a[0] + [0.0, 0.0, 0.1], a[1]), (b[0] + [0.0, 1.5, 0.0], b[1]), (tv, tf))
    v = v + 1e6 if far else v.astype(np.float32)
    offs = np.array([-0.3, 0.0, 0.1, 0.45]) + (1e6 if far else 0.0)
    r, w = check(v, f.astype(fdt), (0, 0, 1), offs, 'spheres and torus far=%s' % far, attr=_colors(v, 3, np.float64 if far else np.float32))
    assert r.v2.dtype == (torch.float64 if far else torch.float32) and r.f2.dtype == torch.int32


def test_oblique_normal_on_dyadic_coordinates_with_planes_through_vertices():
    v, f = R.icosphere(2)
    v = np.round(v * 8) / 8
    c = _clipper(v.astype(np.float32), f)
    h = np.unique(_np(c.split((1, 1, 1), []).vertex_height))
    r, w = check(v.astype(np.float32), f, (1, 1, 1), h, 'dyadic oblique', clipper=c)
    assert r.n_degenerate > 0
    check_parts(r, w, 'dyadic oblique')


def test_oblique_normal_on_random_coordinates():
    rng = np.random.default_rng(11)
    v, f = R.icosphere(2)
    v = v * rng.uniform(0.5, 1.5, (len(v), 1)) + rng.normal(size=3)
    check(v, f, rng.normal(size=3), np.sort(rng.uniform(-2, 2, 23)), 'random oblique', attr=_colors(v, 6, np.float64))
    check(v.astype(np.float32), f, rng.normal(size=3), np.sort(rng.uniform(-2, 2, 700)), 'random oblique fp32, 700 planes')


def test_large_triangle_crossing_1000_planes():
    """One lane loops over 1 001 pieces in the by-face shape; 1 001 lanes share one face in the by-piece shape (``check`` runs both).
    The second mesh puts the long face between short ones, in a second block: the binary search of the by-piece shape crosses it."""
    v = np.array([[0.0, 0.0, 0.0], [1000.5, 0.25, 0.0], [3.0, 900.0, 1.0]])
    r, _ = check(v, np.array([[0, 1, 2]]), (1, 0, 0), np.arange(1000) + 0.5, 'large triangle', attr=_colors(v, 2, np.float64))
    assert r.n_faces == 2001 and r.n_parts == 1001
    sv, sf = R.strip(20, 7)
    v2, f2 = R.merged((sv, sf), (v, np.array([[1, 2, 0]])), (sv + [0, 8, 0], sf[::-1]))
    r, _ = check(v2, f2, (1, 0, 0), np.arange(3000) * 0.25 + 0.125, 'large triangle among small ones, 3000 planes')      # (offsets past LDS)
    assert r.n_parts == 3001


def test_icosphere_5_at_1000_levels():
    v, f = big_sphere()
    r, _ = check(v, f, (0, 0, 1), np.linspace(-0.999, 0.999, 1000), 'sphere 20480 at 1000 levels')
    assert r.n_parts == 1001 and r.n_points > 100_000


def _clip_meshes():
    tv, tf = R.torus(32, 16, 2.0, 0.5)
    tv = tv.astype(np.float64)                  # (the parts of an fp64 mesh carry the cut points unrounded: their borders measure as the sections do)
    a, b = R.icosphere(3), R.icosphere(2, 0.3)
    return (('icosphere(3)', a[0], a[1]), ('torus', tv, tf), ('merged', *R.merged((a[0], a[1]), (b[0] + [3.0, 0.0, 0.2], b[1]), (tv + [0.0, 6.0, 0.0], tf))))


@pytest.mark.parametrize('which', [0, 1, 2])
def test_cross_module_invariants(which):
    """The split mesh keeps the topology; the boundary of part s is the sections of planes s - 1 and s; the areas add up."""
    from nksr_amd.mesh_boundary import MeshBoundary
    from nksr_amd.mesh_slice import MeshSlicer
    from nksr_amd.mesh_topology import MeshTopology
    label, v, f = _clip_meshes()[which]
    offs = np.array([-0.71, -0.2, 0.013, 0.33, 0.64])
    r, w = check(v, f, (0, 0, 1), offs, label)
    t0, t2 = MeshTopology(v, f), MeshTopology(r.v2, r.f2)
    assert t0.is_watertight and t2.is_watertight and t2.euler_characteristic == t0.euler_characteristic
    assert t2.components('edge').n == t0.components('edge').n and t2.invalid_faces == 0 and r.n_degenerate == 0
    s = MeshSlicer(v, f).slice((0, 0, 1), offs)
    start = _np(s.plane_polyline_start)
    pts = _np(s.points64)
    seg = _np(s.segments)
    seg_len = np.sqrt(((pts[seg[:, 1]] - pts[seg[:, 0]]) ** 2).sum(1))
    seg_plane = _np(s.segment_plane)
    p, g = check_parts(r, w, label)
    for j in range(r.n_parts):
        planes = [q for q in (j - 1, j) if 0 <= q < len(offs)]
        loops = MeshBoundary(p[j].v, p[j].f).loops()
        n_poly = sum(start[q + 1] - start[q] for q in planes)
        assert loops.n_loops == n_poly and bool(loops.loop_closed.all()), (label, j, loops.n_loops, n_poly)
        terms = seg_len[np.isin(seg_plane, planes)]
        got, ref = float(_np(loops.loop_length).sum()), math.fsum(terms)
        bound = len(terms) * EPS * math.fsum(np.abs(terms))             # n eps sum |term|: two orders of summing the same n terms
        print('%s part %d: %d loops, length %.6f, err %.3g (bound %.3g)' % (label, j, n_poly, got, abs(got - ref), bound))
        assert abs(got - ref) <= bound
    a2 = R.face_areas(_np(r.v2_64), _np(r.f2))[0]
    a0 = R.face_areas(v, f)[0]
    err, bound = abs(math.fsum(a2) - math.fsum(a0)), float(R.area_bound(v, f, w).sum())
    print('%s: area %.9f, split %.9f, err %.3g (bound %.3g)' % (label, math.fsum(a0), math.fsum(a2), err, bound))
    assert err <= bound
    part_area = [float(R.face_areas(_np(m.v), _np(m.f))[0].sum()) for m in (p[j] for j in range(r.n_parts))]
    assert abs(sum(part_area) - math.fsum(a0)) <= bound + len(a2) * EPS * math.fsum(a2)


def test_grouping_borders_and_arbitrary_labels():
    v, f = R.icosphere(2)
    attr = _colors(v, 3, np.float64)
    r, w = check(v, f, (0, 0, 1), [-0.4, 0.1, 0.5], 'grouping', attr=attr)
    p, g = check_parts(r, w, 'grouping')
    nv = len(v)
    src, vs = _np(p.vertex_source), _np(p.part_vertex_start)
    plane = w['point_plane']
    for j in range(r.n_parts - 1):                      # parts j and j + 1 share exactly the points of plane j, bit for bit
        a, b = p[j], p[j + 1]
        sa, sb = src[vs[j]:vs[j + 1]], src[vs[j + 1]:vs[j + 2]]
        shared = np.intersect1d(sa, sb)
        assert np.array_equal(shared, nv + np.nonzero(plane == j)[0]) and len(shared) > 0
        ia, ib = np.searchsorted(sa, shared), np.searchsorted(sb, shared)
        ia, ib = torch.from_numpy(ia), torch.from_numpy(ib)
        assert torch.equal(_bits(a.v.cpu()[ia]), _bits(b.v.cpu()[ib])) and torch.equal(_bits(a.c.cpu()[ia]), _bits(b.c.cpu()[ib]))
    assert np.all(np.bincount(src[src < nv], minlength=nv) <= 1)       # an original vertex lands in one part
    labels = (np.arange(r.n_faces) * 7 % 5) * 2 + 1                    # labels 1, 3, 5, 7, 9 of 12: the even ones and 10, 11 stay empty
    p2, _ = check_parts(r, w, 'arbitrary labels', labels=labels, n_labels=12)
    assert p2.nonempty == [1, 3, 5, 7, 9] and p2[0].f.shape == (0, 3) and p2[11].v.shape == (0, 3)
    p3 = r.parts(torch.from_numpy(labels))                             # n_labels from the labels: max + 1
    assert len(p3) == 10 and torch.equal(p3.f, p2.f)


def test_clip_keeps_one_side_and_clip_box_a_box():
    from nksr_amd.mesh_clip import MeshClipper
    v, f = R.icosphere(2)
    attr = _colors(v, 3)
    v32 = v.astype(np.float32)
    c = MeshClipper(v32, f, attr)
    r, w = check(v32, f, (0, 1, 1), [0.125], 'clip', attr=attr, clipper=c)
    v2, a2 = _np(r.v2), _np(r.attr2)
    for keep, s in (('below', 0), ('above', 1)):
        _same_mesh(c.clip((0, 1, 1), 0.125, keep=keep), R.compact(v2, w['f2'], w['face_part'] == s, a2))
        _same_mesh(c.clip((0, 1, 1), 0.125, keep=keep), r.part(s))
    cv, cf = R.cube(lo=(-1, -1, -1), size=(2, 2, 2))
    for lo, hi in (((0, 0, 0), (4, 4, 4)), ((-0.5, -2, -0.25), (0.75, 0.5, 3)), ((-3, -3, -3), (3, 3, 3)), ((2, 2, 2), (3, 3, 3))):
        got = MeshClipper(cv, cf, _colors(cv, 2)).clip_box(lo, hi)
        _same_mesh(got, R.clip_box(cv, cf, lo, hi, _colors(cv, 2)))
        print('clip_box', lo, hi, 'V=%d F=%d' % (got.v.shape[0], got.f.shape[0]))
    assert got.f.shape == (0, 3) and got.v.shape == (0, 3)              # (the last box misses the cube)
    sv, sf = R.icosphere(2)
    _same_mesh(MeshClipper(sv, sf).clip_box((-0.3, -2, 0.1), (0.6, 0.7, 2)), R.clip_box(sv, sf, (-0.3, -2, 0.1), (0.6, 0.7, 2)))


def test_hemisphere_area_within_the_chord_error():
    """As test_sphere_section_areas_within_the_chord_error: the mesh lies between the spheres of radius 1 and m = sqrt(1 - e^2 / 3), e its
    longest edge, and it is star-shaped about the centre, so the rays with z >= 0 meet exactly its part with z >= 0: the clipped mesh
    covers the solid angle 2 pi.  A plane patch dA at distance rho from the centre, in a plane at distance d = rho cos(theta), covers
    dOmega = dA cos(theta) / rho^2, so dA = dOmega rho^3 / d with m <= d <= rho <= 1:   2 pi m^2 <= area <= 2 pi / m."""
    v, f = R.icosphere(4)
    e = np.linalg.norm(v[f] - v[np.roll(f, -1, 1)], axis=2).max()
    m = _clipper(v, f).clip((0, 0, 1), 0.0, keep='above')
    area = math.fsum(R.face_areas(_np(m.v), _np(m.f))[0])
    lo, hi = 2 * math.pi * (1 - e * e / 3), 2 * math.pi / math.sqrt(1 - e * e / 3)
    print('hemisphere: area %.9f in [%.9f, %.9f]' % (area, lo, hi))
    assert lo - 1e-12 <= area <= hi + 1e-12 and float(m.v[:, 2].min()) >= -8 * EPS         # (a point: within 4 eps (|a| + |b|) of its plane)


@pytest.mark.parametrize('which', ['strip', 'sphere'])
def test_tiles(which):
    from nksr_amd.mesh_clip import MeshClipper
    if which == 'strip':
        v, f = R.strip(9, 5)
        v = (v @ np.array([[0.96, 0.28, 0.0], [-0.28, 0.96, 0.0], [0.0, 0.0, 1.0]], np.float32).T).astype(np.float32)     # tilted in the plane too
        size, origin, axes = 2.0, (0.25, -0.5), (0, 1)
    else:
        v, f = R.icosphere(4)
        size, origin, axes = 0.4, (0.0, 0.1), (2, 0)
    attr = _colors(v, 3)
    t = MeshClipper(v, f, attr).tiles(size, origin, axes)
    used = np.unique(f)
    levels = [R.interval_levels(v[used, axes[i]].astype(np.float64), size, origin[i]) for i in range(2)]
    for i in range(2):
        assert np.array_equal(t.levels[i], levels[i]) and len(levels[i]) >= 3
    g, v64, c2, (nx, ny) = R.tiles(v, f, levels, axes, attr)
    assert t.shape == (nx, ny) and len(t) == nx * ny and t.tile_index.dtype == torch.int32
    assert np.array_equal(_np(t.tile_index), np.stack(np.divmod(np.arange(nx * ny), ny), 1))
    for name in R.GROUP_ARRAYS:
        got = _np(getattr(t, name))
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    print('tiles %s: %d x %d, %d non-empty, %d faces' % (which, nx, ny, len(t.nonempty), t.f.shape[0]))
    vd = v64.astype(v.dtype)
    bounds = [np.concatenate([[-np.inf], lv, [np.inf]]) for lv in levels]
    worst = 0.0
    for j in range(nx * ny):
        m = t[j]
        _same_mesh(m, R.part_mesh(g, j, vd, c2))
        if m.f.shape[0]:
            ix, iy = divmod(j, ny)
            for i, k in ((0, ix), (1, iy)):            # inside [level k - 1, level k] to the rounding of the points: 4 eps (|a| + |b|) <= 8 eps max |v|
                x = _np(m.v)[:, axes[i]].astype(np.float64)
                tol = 8 * float(np.finfo(v.dtype).eps) * float(np.abs(v).max())
                worst = max(worst, float((bounds[i][k] - x).max()), float((x - bounds[i][k + 1]).max()))
                assert np.all(x >= bounds[i][k] - tol) and np.all(x <= bounds[i][k + 1] + tol), (j, i)
    print('tiles %s: furthest outside its interval %.3g' % (which, worst))
    assert [int(m.f.shape[0]) for m in t] == [int(n) for n in np.diff(g['part_face_start']) if n]


def test_other_entrances_give_the_same_tensors():
    import nksr
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_clip import MeshClipper
    from nksr_amd.mesh_topology import MeshTopology
    v, f = R.torus(48, 24, 2.75, 0.5)
    attr = _colors(v, 3)
    levels = [-0.25, 0.0, 0.25]
    direct = MeshClipper(v, f, attr).split((0, 0, 1), levels)
    assert nksr.metrics.MeshClipper is MeshClipper and nksr.MeshClipper is MeshClipper
    _same_bits(direct, MeshClipper.from_topology(MeshTopology(v, f), attr).split((0, 0, 1), levels))
    mesh = MeshingResult(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(attr).cuda())
    _same_bits(direct, mesh.split((0, 0, 3), levels))
    c = MeshClipper(v, f, attr)
    _same_mesh(mesh.clip((0, 0, 1), 0.1, 'below'), c.clip((0, 0, 1), 0.1, 'below'))
    _same_mesh(mesh.clip_box((-1, -1, -1), (2, 3, 0.2)), c.clip_box((-1, -1, -1), (2, 3, 0.2)))
    a, b = mesh.tiles(1.5, (0.1, 0.2), (0, 1)), c.tiles(1.5, (0.1, 0.2), (0, 1))
    _same_bits(a, b, need=R.GROUP_ARRAYS + ('v64', 'tile_index'))
    with pytest.raises(TypeError):
        MeshClipper.from_topology(mesh)


def test_argument_errors_are_value_errors():
    v, f = R.cube()
    c = _clipper(v, f)
    for normal in ((0, 0, 0), (1, 2), (0, float('nan'), 1), 'up'):
        with pytest.raises(ValueError):
            c.split(normal, [0.5])
    for offsets in ([0.5, 0.5], [1.0, 0.5], [float('inf')], [[0.5]], 'x'):
        with pytest.raises(ValueError):
            c.split((0, 0, 1), offsets)
    for bad in (lambda: c.clip((0, 0, 1), 0.5, keep='both'), lambda: c.clip((0, 0, 1), 'x'), lambda: c.clip((0, 0, 1), float('nan')),
                lambda: c.clip_box((0, 0, 0), (1, 1, 0)), lambda: c.clip_box((0, 0), (1, 1)), lambda: c.clip_box((0, 0, 0), (1, float('inf'), 1)),
                lambda: c.tiles(0.0), lambda: c.tiles(-1.0), lambda: c.tiles(1.0, axes=(0, 0)), lambda: c.tiles(1.0, axes=(0, 3)),
                lambda: c.tiles(1.0, origin=(0.0,)), lambda: c.tiles(1e-9), lambda: _clipper(v, f.astype(np.float32)),
                lambda: _clipper(v, f, attr=np.zeros((7, 3), np.float32)), lambda: _clipper(v, f, attr=np.zeros((8, 3), np.int32)),
                lambda: _clipper(v, f, attr=np.zeros(8, np.float32))):
        with pytest.raises(ValueError):
            bad()
    r = c.split((0, 0, 1), [0.5])
    for labels, k in ((np.zeros(3, np.int64), None), (np.full(r.n_faces, -1), None), (np.full(r.n_faces, 2), 2), (np.zeros(r.n_faces), None)):
        with pytest.raises(ValueError):
            r.parts(labels, k)
    with pytest.raises(IndexError):
        r.parts()[2]
    assert c.split((0, 0, 1), torch.tensor([0.5])).n_faces == 28            # and the clipper still works


def test_recons_tiles_example(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'recons_tiles.py'), '5.0', '60000'], cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    print(out.stdout)
    files = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith('recons_tiles_'))
    assert len(files) >= 4 and 'tiles' in out.stdout and 'border vertices of neighbours coincide: True' in out.stdout
