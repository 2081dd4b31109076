"""The numpy restatement of the mesh cross-sections (tests/mesh_slice_ref.py) against closed forms -- it has to earn its place as the
yardstick of tests/test_gpu_mesh_slice.py -- and the argument errors of the C ABI of csrc/meshslice.hip, which need no GPU."""
import math

import numpy as np
import pytest

import mesh_slice_ref as R


def _slice(v, f, normal, offsets):
    n = R.unit(normal)
    return R.slice_mesh(v, f, n, offsets, R.heights(v, n))


def _tail_once_head_once(r):
    n = r['n_points']
    return (np.array_equal(np.sort(r['segments'][:, 0]), np.arange(n)) and np.array_equal(np.sort(r['segments'][:, 1]), np.arange(n)))


def test_cube_sections_have_the_exact_perimeter_and_area():
    v, f = R.cube((0, 0, 0), (2, 3, 1))
    r = _slice(v, f, (0, 0, 1), [-0.5, 0.25, 0.5, 2.0])
    assert r['n_polylines'] == 2 and r['polyline_closed'].all() and list(r['polyline_plane']) == [1, 2]
    assert list(r['polyline_length']) == [10.0, 10.0] and list(r['polyline_area']) == [6.0, 6.0]       # dyadic: exact
    assert list(r['plane_length']) == [0.0, 10.0, 10.0, 0.0] and list(r['plane_area']) == [0.0, 6.0, 6.0, 0.0] and not r['plane_open'].any()
    assert _tail_once_head_once(r) and r['n_points'] == r['n_segments'] == 2 * 8       # four sides of two triangles per plane
    assert np.all(r['points64'][r['point_plane'] == 1][:, 2] == 0.25)
    # along x, from the other side: the same loop sizes, and still counter-clockwise seen from the normal's tip (a positive area)
    for normal, per, area in (((1, 0, 0), 8.0, 3.0), ((-1, 0, 0), 8.0, 3.0), ((0, 2, 0), 6.0, 2.0)):
        r = _slice(v, f, normal, [0.5 if normal[0] >= 0 else -0.5])
        assert list(r['polyline_length']) == [per] and list(r['polyline_area']) == [area]
    # planes exactly at the vertex heights: the bottom one touches (nothing lies below it), the top one cuts the sides in zero height
    r = _slice(v, f, (0, 0, 1), [0.0, 1.0])
    assert list(r['polyline_plane']) == [1] and list(r['polyline_area']) == [6.0] and list(r['polyline_length']) == [10.0]
    assert r['n_segments'] == 8 and sum(1 for t in r['length_terms'][0] if t == 0.0) == 4     # coincident points at the four top corners
    assert _slice(v, f, (0, 0, 1), [])['n_segments'] == 0


def test_tetrahedron_planes_through_vertices():
    v, f = R.tetrahedron()
    r = _slice(v, f, (0, 0, 1), [-1.0, 0.0, 0.5, 1.0, 2.0])
    # z = 0: three vertices in the plane, that face is all above and nothing is below -> no crossing; z = 1: the apex alone is above
    assert list(r['polyline_plane']) == [2, 3] and r['polyline_closed'].all()
    assert r['polyline_area'][0] == 0.125 and r['polyline_area'][1] == 0.0 and r['polyline_length'][1] == 0.0
    assert abs(r['polyline_length'][0] - (1.0 + math.sqrt(0.5))) < 1e-15
    # along (1, 1, 0), at the height of vertices 1 and 2: the plane holds that edge, the other two vertices lie below it -- a loop that
    # runs along the edge and back
    n = R.unit((1, 1, 0))
    h = R.heights(v, n)
    assert h[1] == h[2] > h[0] == h[3]
    r = R.slice_mesh(v, f, n, [h[1]], h)
    assert r['n_polylines'] == 1 and r['polyline_closed'][0] and _tail_once_head_once(r) and r['n_segments'] == 4
    assert abs(r['polyline_length'][0] - 2.0 * math.sqrt(2.0)) < 1e-15 and r['polyline_area'][0] == 0.0


def test_torus_loop_counts_and_signs():
    v, f = R.torus(48, 24, 2.75, 0.5)
    zs = [-0.3, 0.0, 0.1, 0.45]
    r = _slice(v, f, (0, 0, 1), zs)
    assert r['n_polylines'] == 8 and r['polyline_closed'].all() and _tail_once_head_once(r) and not r['plane_open'].any()
    for j, z in enumerate(zs):
        ids = r['plane_polyline_start'][j:j + 2]
        a = r['polyline_area'][ids[0]:ids[1]]
        assert len(a) == 2 and a.max() > 0 > a.min()                                   # the outer loop and the hole
        w = math.sqrt(0.25 - z * z)
        exact = math.pi * ((2.75 + w) ** 2 - (2.75 - w) ** 2)
        # inscribed polygons, a little less than the annulus: the 48-gon round the axis loses 1 - sinc(2 pi / 48) < 0.3 %, the 24-gon of
        # the tube pulls the half-width w in by at most its sagitta r (1 - cos(pi / 24)) times r / w (twice that allowed)
        tol = 0.003 + 2.0 * 0.5 * (1.0 - math.cos(math.pi / 24)) * 0.5 / (w * w)
        assert (1.0 - tol) * exact < r['plane_area'][j] < exact
        assert abs(a.max() - math.pi * (2.75 + w) ** 2) < 0.03 * a.max()
    # across the ring (normal x, through the centre): two discs
    r = _slice(v, f, (1, 0, 0), [0.01])
    assert r['n_polylines'] == 2 and (r['polyline_area'] > 0).all() and abs(r['plane_area'][0] - 2 * math.pi * 0.25) < 0.05


def test_open_chains_on_a_strip():
    v, f = R.strip(4, 3)
    r = _slice(v, f, (1, 0, 0), [0.5, 1.5, 2.0])
    assert r['n_polylines'] == 3 and not r['polyline_closed'].any() and list(r['plane_open']) == [1, 1, 1]
    assert list(r['polyline_length']) == [3.0, 3.0, 3.0] and not r['polyline_area'].any() and not r['plane_area'].any()
    assert list(np.diff(r['polyline_start'])) == [7, 7, 7]                             # m + 1 points for m = 6 segments
    pts = r['points64'][r['polyline_points'][:7]]
    assert pts[0, 1] == 3.0 and pts[-1, 1] == 0.0 and np.all(pts[:, 0] == 0.5)           # n x n_face: towards -y
    assert list(r['segment_rank'][r['polyline_rep']]) == [0, 0, 0] and (r['pred'][r['polyline_rep']] == -1).all()


def test_chains_end_at_nonmanifold_and_misoriented_edges():
    import mesh_topology_ref as T
    v, f = T.three_fan()
    r = _slice(v, f, (1, 0, 0), [0.25])
    assert r['n_segments'] == 3 and r['n_polylines'] == 3 and (r['succ'] == -1).all() and list(r['plane_open']) == [3]
    v, f = R.cube()
    g = f.copy()
    g[4] = g[4][[0, 2, 1]]
    a, b = _slice(v, f, (0, 0, 1), [0.5]), _slice(v, g, (0, 0, 1), [0.5])
    assert a['n_polylines'] == 1 and b['n_polylines'] > 1 and b['n_segments'] == a['n_segments'] and not b['polyline_closed'].all()


def test_slice_c_abi_argument_errors_without_a_gpu():
    import ctypes as C
    from nksr_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    A, Z = C.cast(buf, C.c_void_p), None

    def err():
        return lib.nksr_last_error().decode()

    assert lib.nksr_slice_heights(A, 0, 3, Z, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_heights(Z, 0, 0, A, Z, Z) == 0
    assert lib.nksr_slice_heights(A, 0, -1, A, A, Z) != 0 and 'negative' in err()
    assert lib.nksr_slice_counts(A, 3, A, 0, 1, A, A, 3, A, 1, A, Z, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_counts(A, 3, A, 0, 1, A, A, 4, A, 1, A, A, A, A, Z) != 0 and 'n_edges' in err()
    assert lib.nksr_slice_counts(A, 3, A, 0, 1, A, A, 3, A, 1 << 31, A, A, A, A, Z) != 0 and 'n_planes' in err()
    assert lib.nksr_slice_points(A, 0, 3, A, A, 3, A, 1, A, A, 1 << 31, 0, A, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_slice_points(A, 0, 3, A, A, 3, A, 1, A, A, 2, 1, Z, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_points(Z, 0, 3, Z, Z, 3, Z, 1, Z, Z, 0, 1, Z, Z, Z, Z) == 0
    assert lib.nksr_slice_segments(A, 3, A, 0, 1, A, 1, A, A, A, A, A, A, A, 1, A, A, A, A, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_segments(A, 3, A, 0, 1, A, 1, A, A, A, A, A, A, A, 1 << 31, A, A, A, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_slice_segments(Z, 3, Z, 0, 0, Z, 0, Z, Z, Z, Z, Z, Z, Z, 0, Z, Z, Z, Z, Z, Z) == 0
    assert lib.nksr_chain_rank(A, 4, A, A, A, A, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_chain_rank(A, 4, Z, A, A, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_chain_rank(A, 4, C.c_void_p(C.addressof(buf) + 8), A, A, A, A, Z) != 0 and ('aligned' in err() or C.addressof(buf) % 16 == 8)
    assert lib.nksr_chain_rank(A, 1 << 31, A, A, A, A, A, Z) != 0 and '2^31' in err()
    assert [lib.nksr_chain_rank_rounds(n) for n in (0, 1, 2, 3, 4, 5, 6000, 1 << 20)] == [1, 1, 2, 3, 3, 4, 14, 21]
    assert lib.nksr_slice_rep_list(A, A, 4, A, 5, A, A, Z) != 0 and 'polylines' in err()
    assert lib.nksr_slice_rep_list(A, A, 4, Z, 2, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_polyline_sizes(A, A, A, A, 4, A, A, 2, A, Z, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_polyline_sizes(A, A, A, A, 4, A, Z, 2, A, A, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_polylines(A, A, A, A, 4, A, A, A, A, 2, A, 4, Z, A, A, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_slice_polylines(A, A, A, A, 4, A, A, A, A, 5, A, 4, A, A, A, A, A, Z) != 0 and 'polylines' in err()
    assert lib.nksr_slice_polylines(Z, Z, Z, Z, 0, Z, Z, Z, Z, 0, Z, 0, Z, Z, Z, Z, Z, Z) == 0


def test_mesh_slicer_is_exported_and_documented():
    import nksr
    from nksr_amd import build
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_slice import MeshSlicer
    assert 'MeshSlicer' in nksr.__all__ and nksr.MeshSlicer is MeshSlicer and nksr.metrics.MeshSlicer is MeshSlicer
    assert 'meshslice.hip' in build.SOURCES and callable(MeshingResult.slice) and callable(MeshingResult.contours)
    assert callable(nksr.utils.write_obj_polylines)
    assert 'bit for bit' in __import__('nksr_amd.mesh_slice').mesh_slice.__doc__


def test_write_obj_polylines_round_trips(tmp_path):
    import nksr
    pts = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, 1e-9], [5, 5, 5]], np.float64)
    start, ids = np.array([0, 3, 5]), np.array([3, 0, 1, 4, 2])
    path = str(tmp_path / 'lines.obj')
    nksr.utils.write_obj_polylines(path, pts, start, ids)
    vs, ls = [], []
    for line in open(path):
        w = line.split()
        if w and w[0] == 'v':
            vs.append([float(x) for x in w[1:]])
        elif w and w[0] == 'l':
            ls.append([int(x) - 1 for x in w[1:]])
    assert np.array_equal(np.array(vs), pts) and ls == [[3, 0, 1], [4, 2]]
    with pytest.raises(ValueError):
        nksr.utils.write_obj_polylines(path, pts, np.array([0, 9]), ids)
