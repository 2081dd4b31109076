"""Mesh boundary loops and hole filling on the MI355X (nksr_amd/mesh_boundary.py, csrc/meshbound.hip) against the numpy restatement
(tests/mesh_boundary_ref.py).  Every integer array is compared index for index, nothing left out and nothing masked; the measures within
the bounds derived at ``check``, against math.fsum of the terms the restatement evaluates from the vertices.  Every comparison prints
its largest error before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_boundary_ref as R
import mesh_topology_ref as T

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def _boundary(v, f):
    from nksr_amd.mesh_boundary import MeshBoundary
    return MeshBoundary(v, f)


def _np(x):
    return x.cpu().numpy()


def _host(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def _tensors(r):
    return {k: x for k, x in vars(r).items() if isinstance(x, torch.Tensor)}


def _same_bits(a, b):
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb) and set(R.INTEGER_ARRAYS) | set(R.FLOAT_ARRAYS) <= set(ta)
    for k in ta:
        x, y = ta[k], tb[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


def _sum_bound(terms):
    """(math.fsum(terms), n eps sum |term|): a sum of n terms in any order is within (n - 1) eps sum |term| of the exact one (each of
    the n - 1 additions rounds a partial sum that is at most sum |term|, to first order), and fsum is the exact one rounded once."""
    return math.fsum(terms), len(terms) * EPS * math.fsum(abs(t) for t in terms)


def check(v, f, label, boundary=None):
    """``MeshBoundary.loops`` against the restatement.  Bounds, per loop of n edges:
      length, area vector   |sum - fsum(terms)| <= n eps sum |term| (``_sum_bound``); the terms are bit for bit the kernel's: every
                            operation is rounded on its own on both sides
      area                  the norm of a vector within d (per component) of the reference's is within |d|_1 of its norm; three products,
                            two sums and a root add at most 4 eps of the norm
      centroid              c = p0 + S / W per axis, S the moment sum (bound dS as above), W the length (bound dW):
                            |S / W - S* / W*| <= (dS + |S* / W*| dW) / (W* - dW); the division rounds once (eps of the quotient, as does
                            the reference's), the final add once (eps |c|, as does the reference's).  Everything but that last rounding
                            is relative to the loop's extent, not to the size of the coordinates.
      box                   exact: minima and maxima of the coordinates themselves"""
    b = boundary or _boundary(v, f)
    r = b.loops()
    want = R.boundary_loops(_host(v), _host(f))
    print('%s: B=%d L=%d' % (label, r.n_boundary, r.n_loops))
    assert (r.n_boundary, r.n_loops) == (want['n_boundary'], want['n_loops']) and r.n_boundary == b.topology.boundary_edges
    for k in R.INTEGER_ARRAYS:
        got = _np(getattr(r, k))
        assert got.shape == want[k].shape, (label, k, got.shape, want[k].shape)
        assert np.array_equal(got, want[k]), (label, k)
        assert got.dtype == (bool if k in ('loop_closed', 'loop_simple') else np.int32), (label, k, got.dtype)
    assert int(_np(r.loop_edges).sum()) == r.n_boundary                 # no half-edge is lost
    nl = r.n_loops
    for k in R.FLOAT_ARRAYS:
        assert getattr(r, k).dtype == torch.float64 and getattr(r, k).shape == want[k].shape, (label, k)
    length, vec, area, cen = _np(r.loop_length), _np(r.loop_area_vector), _np(r.loop_area), _np(r.loop_centroid)
    worst = dict(length=(0.0, 0.0), vector=(0.0, 0.0), area=(0.0, 0.0), centroid=(0.0, 0.0))       # name -> (largest error, the bound there)

    def note(name, err, bound):
        if err >= worst[name][0]:
            worst[name] = (err, bound)
    for l in range(nl):
        w_ref, dw = _sum_bound(want['length_terms'][l])
        note('length', abs(length[l] - w_ref), dw)
        assert abs(length[l] - w_ref) <= dw, (label, 'length', l, length[l], w_ref, dw)
        dvec = 0.0
        for a in range(3):
            ref, d = _sum_bound(want['area_terms'][l][a])
            note('vector', abs(vec[l, a] - ref), d)
            assert abs(vec[l, a] - ref) <= d, (label, 'area vector', l, a, vec[l, a], ref, d)
            dvec += d
        d = dvec + 4 * EPS * want['loop_area'][l]
        note('area', abs(area[l] - want['loop_area'][l]), d)
        assert abs(area[l] - want['loop_area'][l]) <= d, (label, 'area', l, area[l], want['loop_area'][l], d)
        for a in range(3):
            s_ref, ds = _sum_bound(want['moment_terms'][l][a])
            if w_ref > 0:
                q = s_ref / w_ref
                d = (ds + abs(q) * dw) / (w_ref - dw) + 2 * EPS * abs(q) + 2 * EPS * abs(want['loop_centroid'][l, a])
            else:
                d = 0.0
            note('centroid', abs(cen[l, a] - want['loop_centroid'][l, a]), d)
            assert abs(cen[l, a] - want['loop_centroid'][l, a]) <= d, (label, 'centroid', l, a, cen[l, a], want['loop_centroid'][l, a], d)
    print('%s: largest error (bound there): %s' % (label, ', '.join('%s %.3g (%.3g)' % (k, e, d) for k, (e, d) in worst.items())))
    assert np.array_equal(_np(r.loop_box), want['loop_box']), (label, 'box')
    assert not vec[~want['loop_closed']].any()
    for kw in ({}, {'max_edges': 6}, {'max_length': 4.0, 'simple_only': False}, {'max_area': 1.0}):
        got = r.select(**kw)
        assert got.dtype == torch.bool and np.array_equal(_np(got), R.select(want, **kw)), (label, kw)
        assert not _np(got)[~want['loop_closed']].any()
    return b, r, want


def check_fill(b, v, f, want, keep, method, label, colors=None):
    """``fill`` against the restatement: every integer array index for index, the old rows bit for bit, the new vertices equal to the
    centroids the GPU reports cast once, the colours of new vertices within n eps sum |c| / n of fsum(c) / n plus one rounding of the
    division and one of the cast (2^-24 for fp32 colours)."""
    v, f = _host(v), _host(f)
    v2, f2, c2, mask, face_loop = b.fill(torch.from_numpy(np.asarray(keep)), method, None if colors is None else torch.from_numpy(colors))
    w_v2, w_f2, w_c2, w_mask, w_loop, colour_terms = R.fill(v, f, want, keep, method, colors)
    assert v2.dtype == b.v.dtype and f2.dtype == b.f.dtype and mask.dtype == torch.bool and face_loop.dtype == torch.int32
    assert np.array_equal(_np(f2), w_f2.astype(_np(f2).dtype)) and np.array_equal(_np(face_loop), w_loop) and np.array_equal(_np(mask), w_mask), label
    nv, nf = len(v), len(f)
    assert torch.equal(v2[:nv].cpu(), torch.from_numpy(v)) and torch.equal(f2[:nf].cpu(), torch.from_numpy(f).to(f2.dtype)), label
    kept = np.nonzero(keep)[0]
    if method == 'centroid':
        assert torch.equal(v2[nv:], b.loops().loop_centroid[torch.from_numpy(kept).to(v2.device)].to(v2.dtype)), label
    else:
        assert v2.shape[0] == nv
    if colors is not None:
        assert c2.dtype == torch.float32 and torch.equal(c2[:nv].cpu(), torch.from_numpy(colors))
        err = bound = 0.0
        for j, per in enumerate(colour_terms):
            for ch, terms in enumerate(per):
                s, ds = _sum_bound(terms)
                mean = s / len(terms)
                d = ds / len(terms) + EPS * abs(mean) + 2.0 ** -24 * abs(mean)
                e = abs(float(c2[nv + j, ch]) - mean)
                err, bound = max(err, e), max(bound, d)
                assert e <= d, (label, 'colour', j, ch, e, d)
        print('%s: colours max err %.3g (largest bound %.3g)' % (label, err, bound))
    else:
        assert c2 is None
    return v2, f2, c2, mask, face_loop


def _watertight(v2, f2):
    from nksr_amd.mesh_topology import MeshTopology
    return MeshTopology(v2, f2)


def test_closed_forms_triangle_tetrahedron_cube():
    v, f = R.triangle()
    b, r, w = check(v, f, 'triangle')
    assert r.n_loops == 1 and _np(r.loop_vertices).tolist() == [0, 1, 2] and _np(r.loop_area).tolist() == [0.5]
    v2, f2, _, _, _ = check_fill(b, v, f, w, [True], 'fan', 'triangle fan')
    t = _watertight(v2, f2)
    assert t.is_watertight and _np(f2).tolist() == [[0, 1, 2], [2, 1, 0]]                 # the closed two-face pillow
    v, f = R.open_tetrahedron()
    b, r, w = check(v, f, 'tetrahedron less a face')
    for method in ('fan', 'centroid'):
        t = _watertight(*check_fill(b, v, f, w, [True], method, 'tetrahedron ' + method)[:2])
        assert t.is_watertight and t.euler_characteristic == 2
    v, f = R.open_cube()
    b, r, w = check(v, f, 'cube less a side')
    assert _np(r.loop_edges).tolist() == [4] and _np(r.loop_length).tolist() == [4.0] and _np(r.loop_area).tolist() == [1.0]
    assert _np(r.loop_centroid).tolist() == [[0.5, 0.5, 1.0]] and _np(r.loop_box).tolist() == [[0, 0, 1, 1, 1, 1]]
    assert _watertight(*check_fill(b, v, f, w, [True], 'centroid', 'cube centroid')[:2]).is_watertight


def test_closed_and_empty_meshes():
    for label, (v, f) in (('sphere', R.icosphere(2)), ('F = 0', (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32))),
                          ('V = 0', (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)))):
        b, r, w = check(v, f, label)
        assert r.n_boundary == 0 and r.n_loops == 0 and _np(r.loop_start).tolist() == [0] and r.loop_centroid.shape == (0, 3)
        for method in ('fan', 'centroid'):
            v2, f2, _, mask, face_loop = check_fill(b, v, f, w, np.zeros(0, bool), method, label)
            assert v2.shape == tuple(v.shape) and f2.shape == tuple(f.shape) and face_loop.shape == (0,) and not mask.any()


def test_umbrella_walk_at_vertices_where_borders_touch():
    """Two welded cubes opened at the common corner: two loops (one fan of faces each).  The strip less two diagonally adjacent quads
    and the pinched disc: the surface is pinched at the vertex, and the definition gives ONE loop that passes it twice -- for the strip
    a loop of 8, not two of 4 (see tests/test_mesh_boundary_cpu.py)."""
    v, f, shared = R.two_cubes_opened_at_the_shared_vertex()
    b, r, w = check(v, f, 'two cubes')
    assert _np(r.loop_edges).tolist() == [3, 3] and (_np(r.loop_vertices) == shared).sum() == 2 and _np(r.loop_simple).all()
    assert _watertight(*check_fill(b, v, f, w, [True, True], 'fan', 'two cubes fan')[:2]).boundary_edges == 0
    v, f, shared = R.strip_less_two_quads()
    b, r, w = check(v, f, 'strip less two quads')
    assert sorted(_np(r.loop_edges).tolist()) == [8, 16] and sorted(_np(r.loop_simple).tolist()) == [False, True]
    v, f = R.pinched_disc(4)
    b, r, w = check(v, f, 'pinched disc')
    assert r.n_loops == 1 and _np(r.loop_edges).tolist() == [10] and not _np(r.loop_simple).any() and not _np(r.select()).any()
    with pytest.raises(ValueError):
        b.fill([True], 'fan')
    check_fill(b, v, f, w, [True], 'centroid', 'pinched disc centroid')
    assert b.fill([True], 'centroid')[1].shape[0] == len(f) + 10


def test_walk_of_999_steps_about_one_centre():
    v, f = R.disc_fan(1000)
    b, r, w = check(v, f, 'disc fan')
    assert max(w['walk_steps']) == 999 and _np(r.loop_edges).tolist() == [1002] and _np(r.loop_closed).all()


def test_open_borders():
    """Non-manifold and misoriented edges end chains; invalid faces and unreferenced vertices take no part."""
    v, f = R.three_fan()
    b, r, w = check(v, f, 'three fan')
    assert r.n_loops == 3 and not _np(r.loop_closed).any() and np.diff(_np(r.loop_start)).tolist() == [3, 3, 3]
    with pytest.raises(ValueError):
        b.fill([True, False, False])
    v, f = R.icosphere(1)
    ring = np.unique(f[(f == 0).any(1)])
    g = f[~(f == 0).any(1)].copy()
    flip = int(np.nonzero(np.isin(g, ring).any(1))[0][0])                   # a face at the hole's border
    g[flip] = g[flip][[0, 2, 1]]
    b, r, w = check(v, g, 'holed sphere, one face flipped')
    assert b.topology.misoriented_edges > 0 and not _np(r.loop_closed).all()
    v, f = R.random_soup(60, 20)
    b, r, w = check(v, f, 'random soup')
    assert r.n_boundary > 0
    v, f = R.open_cube()
    v = np.concatenate([v, [[5, 5, 5], [6, 6, 6]]]).astype(np.float32)
    g = np.concatenate([f[:3], [[0, 99, 3], [-1, 2, 3]], f[3:], [[4, 4, 7]]])
    b, r, w = check(v, g, 'invalid faces and unreferenced vertices')
    assert r.n_loops == 1 and _np(r.loop_edges).tolist() == [4] and not np.isin(_np(r.face), [3, 4, len(g) - 1]).any()


def test_long_loops_with_the_smallest_id_in_the_middle():
    v, f = R.cylinder(6000, 1)
    b, r, w = check(v, f, 'cylinder')
    assert _np(r.loop_edges).tolist() == [6000, 6000] and _np(r.loop_closed).all() and r.rounds == 15
    rep = w['loop_rep']
    assert (w['boundary_rank'][w['pred'][rep]] == 5999).all() and (w['boundary_rank'][w['succ'][rep]] == 1).all()
    assert np.abs(w['face'][rep] - w['face'][w['pred'][rep]]).max() > 1000            # the face order is rolled: a loop's smallest id lies mid-loop
    assert np.all(np.abs(_np(r.loop_area) - math.pi) < 1e-5) and np.all(np.abs(_np(r.loop_length) - 2 * math.pi) < 1e-5)
    _same_bits(r, _boundary(v, f).loops())


@pytest.mark.parametrize('n_boundary', [63, 64, 65, 255, 256, 257])
def test_launch_edges_and_determinism(n_boundary):
    v, f = R.triangle_strip(n_boundary - 2)
    v, f = T.shuffled(v, f, n_boundary)
    b, r, w = check(v, f, 'strip of %d' % n_boundary)
    assert r.n_boundary == n_boundary and r.n_loops == 1
    _same_bits(r, _boundary(v, f).loops())
    a, c = b.fill(r.select(), 'centroid'), _boundary(v, f).fill(r.select(), 'centroid')
    assert all(torch.equal(x, y) for x, y in zip(a, c) if x is not None)


@pytest.mark.parametrize('fdt', [np.int32, np.int64])
@pytest.mark.parametrize('kind', ['fp32', 'fp64', 'far', 'torch'])
def test_types(fdt, kind):
    """fp32, fp64 and fp64 coordinates near 1e6 (the centroid's bound stays relative to the loop's extent up to the final rounding),
    numpy and torch inputs, int32 and int64 faces."""
    v, f = R.strip_less_two_quads(5, 4)[:2]
    v = v.astype(np.float64) * 0.37 + (1e6 if kind == 'far' else 0.0)
    v = v.astype(np.float32) if kind in ('fp32', 'torch') else v
    f = f.astype(fdt)
    vin, fin = (torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()) if kind == 'torch' else (v, f)
    b, r, w = check(vin, fin, 'types %s %s' % (kind, fdt.__name__))
    if kind == 'far':
        extent = (w['loop_box'][:, 3:] - w['loop_box'][:, :3]).max()
        err = np.abs(_np(r.loop_centroid) - w['loop_centroid']).max()
        print('far: centroid err %.3g, extent %.3g, ulp(1e6) %.3g' % (err, extent, 2.0 ** -33))
        assert err <= 2.0 ** -33 + 64 * EPS * extent                   # one rounding at 1e6, the rest relative to the extent
    keep = R.select(w)
    for method in ('centroid', 'fan'):
        v2, f2, _, _, _ = check_fill(b, vin, fin, w, keep, method, 'types fill ' + method)
        assert f2.dtype == (torch.int32 if fdt == np.int32 else torch.int64) and v2.dtype == (torch.float64 if kind in ('fp64', 'far') else torch.float32)


@functools.lru_cache(maxsize=None)
def holed_sphere():
    v, f = R.holed_icosphere(3, 12)
    colors = np.random.RandomState(1).uniform(0, 1, (len(v), 3)).astype(np.float32)
    return v, f, colors


@pytest.mark.parametrize('method', ['centroid', 'fan'])
def test_fill_invariants_on_a_sphere_with_a_dozen_holes(method):
    from nksr_amd.fields.base_field import MeshingResult
    v, f, colors = holed_sphere()
    b, r, w = check(v, f, 'holed sphere')
    assert r.n_loops == 12 and w['loop_closed'].all() and w['loop_simple'].all() and sorted(set(w['loop_edges'])) == [5, 6]
    keep = R.select(w)
    assert keep.all()
    v2, f2, c2, mask, face_loop = check_fill(b, v, f, w, keep, method, 'holed sphere ' + method, colors)
    t = _watertight(v2, f2)
    assert t.is_watertight and t.euler_characteristic == 2 and t.invalid_faces == 0
    p = _np(v2)[_np(f2)[len(f):]]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    radial = (normal * p.mean(1)).sum(1)
    print('new faces: smallest normal . radial %.3g' % radial.min())
    assert np.all(radial > 0)
    # a threshold under the largest hole: exactly the loops at or under it, and the border shrinks by their edges
    small = R.select(w, max_edges=5)
    assert 0 < small.sum() < 12 and np.array_equal(_np(r.select(max_edges=5)), small)
    v3, f3, _, _, _ = check_fill(b, v, f, w, small, method, 'holed sphere, max_edges=5 ' + method)
    t3 = _watertight(v3, f3)
    assert t3.boundary_edges == b.topology.boundary_edges - int(w['loop_edges'][small].sum()) and t3.is_oriented and t3.is_edge_manifold
    left = _boundary(v3, f3).loops()
    assert left.n_loops == 12 - small.sum() and (_np(left.loop_edges) == 6).all()
    # MeshingResult.fill_holes equals the direct call
    mesh = MeshingResult(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(colors).cuda())
    filled = mesh.fill_holes(max_edges=5, method=method)
    direct = b.fill(r.select(max_edges=5), method, colors)
    assert torch.equal(filled.v.view(torch.int64), direct[0].view(torch.int64)) and torch.equal(filled.f, direct[1]) and torch.equal(filled.c, direct[2])
    _same_bits(mesh.boundary_loops(), r)


def test_other_entrances_and_argument_errors():
    from nksr_amd.mesh_boundary import MeshBoundary
    from nksr_amd.mesh_slice import MeshSlicer, halfedge_edges
    from nksr_amd.mesh_topology import MeshTopology
    v, f, _ = holed_sphere()
    topo = MeshTopology(v, f)
    b = MeshBoundary.from_topology(topo)
    assert b.topology is topo and b.loops() is b.loops()
    _same_bits(b.loops(), MeshBoundary(v, f).loops())
    he = topo.halfedge_edge
    assert he is topo.halfedge_edge and MeshSlicer.from_topology(topo).halfedge_edge is he
    assert torch.equal(he, halfedge_edges(topo._keys_sorted, topo._ids_sorted, topo.n_vertices)) and he.dtype == torch.int32
    want = T.edge_table(f, len(v))
    edge_of = {(int(a), int(c)): e for e, (a, c) in enumerate(want['edges'])}
    ends = np.stack([f, np.roll(f, -1, 1)], -1).reshape(-1, 2)
    assert _np(he).tolist() == [edge_of[(min(a, c), max(a, c))] for a, c in ends]
    with pytest.raises(TypeError):
        MeshBoundary.from_topology(b)
    r = b.loops()
    for bad in (dict(method='ear'), dict(keep=[True])):
        with pytest.raises(ValueError):
            b.fill(bad.get('keep', r.select()), bad.get('method', 'fan'))
    with pytest.raises(ValueError):
        b.fill(r.select(), 'centroid', colors=np.zeros((3, 3), np.float32))
    for kw in ({'max_edges': -1}, {'max_length': float('nan')}, {'max_area': 'big'}):
        with pytest.raises(ValueError):
            r.select(**kw)
    with pytest.raises(ValueError):
        MeshBoundary(v, f.astype(np.float32))
    assert b.fill(r.select(), 'fan')[1].shape[0] == len(f) + int((_np(r.loop_edges) - 2).sum())        # and it still works
