"""The numpy restatement of the mesh boundary loops (tests/mesh_boundary_ref.py) against closed forms -- it has to earn its place as the
yardstick of tests/test_gpu_mesh_boundary.py -- the exports, and the argument errors of the C ABI of csrc/meshbound.hip, which need no
GPU."""
import math

import numpy as np
import pytest

import mesh_boundary_ref as R
import mesh_topology_ref as T


def _watertight(v, f):
    t = T.edge_table(f, len(v))
    return t['boundary_edges'] == 0 and t['nonmanifold_edges'] == 0 and t['misoriented_edges'] == 0 and t['invalid_faces'] == 0


def test_single_triangle_and_its_fan_pillow():
    v, f = R.triangle()
    r = R.boundary_loops(v, f)
    assert r['n_boundary'] == 3 and r['n_loops'] == 1 and r['loop_closed'].all() and r['loop_simple'].all()
    assert list(r['loop_vertices']) == [0, 1, 2] and list(r['succ']) == [1, 2, 0] and list(r['pred']) == [2, 0, 1]
    assert r['loop_area'][0] == 0.5 and list(r['loop_area_vector'][0]) == [0.0, 0.0, 0.5]
    assert abs(r['loop_length'][0] - (2.0 + math.sqrt(2.0))) < 1e-15
    v2, f2, _, mask, face_loop, _ = R.fill(v, f, r, R.select(r), 'fan')
    assert len(v2) == 3 and not mask.any() and f2.tolist() == [[0, 1, 2], [2, 1, 0]] and list(face_loop) == [0] and _watertight(v2, f2)
    v2, f2, _, mask, face_loop, _ = R.fill(v, f, r, R.select(r), 'centroid')
    assert len(v2) == 4 and list(mask) == [False] * 3 + [True] and f2[1:].tolist() == [[1, 0, 3], [2, 1, 3], [0, 2, 3]] and _watertight(v2, f2)


def test_open_tetrahedron_and_open_cube_have_the_exact_measures():
    v, f = R.open_tetrahedron()
    r = R.boundary_loops(v, f)
    assert r['n_loops'] == 1 and list(r['loop_edges']) == [3] and sorted(r['loop_vertices']) == [0, 2, 3]
    for method in ('fan', 'centroid'):
        v2, f2 = R.fill(v, f, r, R.select(r), method)[:2]
        assert _watertight(v2, f2) and T.edge_table(f2, len(v2))['euler'] == 2
    v, f = R.open_cube()
    r = R.boundary_loops(v, f)
    assert r['n_loops'] == 1 and list(r['loop_edges']) == [4] and list(r['loop_length']) == [4.0] and list(r['loop_area']) == [1.0]
    assert list(r['loop_centroid'][0]) == [0.5, 0.5, 1.0] and list(r['loop_box'][0]) == [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    assert r['loop_area_vector'][0, 2] == -1.0              # the border runs with its faces: clockwise seen from outside the hole
    v2, f2 = R.fill(v, f, r, R.select(r), 'centroid')[:2]
    assert _watertight(v2, f2) and list(v2[-1]) == [0.5, 0.5, 1.0] and len(f2) == len(f) + 4


def test_closed_and_empty_meshes_have_no_loops():
    for v, f in (R.icosphere(1), (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int64)), (np.zeros((0, 3)), np.zeros((0, 3), np.int64))):
        r = R.boundary_loops(v, f)
        assert r['n_boundary'] == 0 and r['n_loops'] == 0 and list(r['loop_start']) == [0] and r['loop_centroid'].shape == (0, 3)
        v2, f2 = R.fill(v, f, r, R.select(r), 'centroid')[:2]
        assert v2.shape == np.asarray(v).shape and f2.shape == f.shape


def test_borders_that_touch_in_a_vertex():
    """The rotation about the head stays inside one fan of faces.  Two borders that meet in a vertex whose faces form ONE fan each --
    the two welded cubes -- are two loops.  Where the SURFACE is pinched -- the strip less two diagonally adjacent quads leaves two
    fans of faces at the shared vertex, exactly as the pinched disc does -- each fan leads from one hole into the other, and the
    definition gives one loop of 8 that passes the vertex twice, not two loops of 4: the connectivity alone cannot tell the two
    cases apart, so the loop is reported as not simple and ``select`` leaves it out by default."""
    v, f, shared = R.strip_less_two_quads()
    r = R.boundary_loops(v, f)
    assert sorted(r['loop_edges']) == [8, 16] and r['loop_closed'].all() and sorted(r['loop_simple']) == [False, True]
    knot = int(np.nonzero(~r['loop_simple'])[0][0])
    ids = list(r['loop_vertices'][r['loop_start'][knot]:r['loop_start'][knot + 1]])
    assert len(ids) == 8 and ids.count(shared) == 2 and len(set(ids)) == 7 and list(R.select(r)) == [k != knot for k in range(2)]
    v, f, shared = R.two_cubes_opened_at_the_shared_vertex()
    r = R.boundary_loops(v, f)
    assert list(r['loop_edges']) == [3, 3] and all(shared in r['loop_vertices'][r['loop_start'][l]:r['loop_start'][l + 1]] for l in (0, 1))
    v2, f2 = R.fill(v, f, r, R.select(r), 'fan')[:2]
    assert T.edge_table(f2, len(v2))['boundary_edges'] == 0


def test_long_umbrella_and_pinched_disc():
    v, f = R.disc_fan(1000)
    r = R.boundary_loops(v, f)
    assert r['n_loops'] == 1 and list(r['loop_edges']) == [1002] and max(r['walk_steps']) == 999 and r['loop_simple'].all()
    assert abs(r['loop_area'][0] - math.pi) < 0.01
    v, f = R.pinched_disc(4)
    r = R.boundary_loops(v, f)
    assert r['n_loops'] == 1 and list(r['loop_edges']) == [10] and r['loop_closed'].all() and not r['loop_simple'].any()
    assert list(r['loop_vertices']).count(0) == 2 and not R.select(r).any() and R.select(r, simple_only=False).all()
    with pytest.raises(ValueError):
        R.fill(v, f, r, [True], 'fan')
    assert len(R.fill(v, f, r, [True], 'centroid')[1]) == len(f) + 10


def test_open_borders_end_at_nonmanifold_and_misoriented_edges():
    v, f = R.three_fan()
    r = R.boundary_loops(v, f)
    assert r['n_boundary'] == 6 and r['n_loops'] == 3 and not r['loop_closed'].any() and list(r['loop_edges']) == [2, 2, 2]
    assert not R.select(r).any() and not r['loop_area_vector'].any() and list(np.diff(r['loop_start'])) == [3, 3, 3]
    with pytest.raises(ValueError):
        R.fill(v, f, r, [True, False, False])
    v, f = R.random_soup(60, 20)
    r = R.boundary_loops(v, f)
    assert r['loop_edges'].sum() == r['n_boundary'] > 0 and not R.select(r)[~r['loop_closed']].any()


def test_boundary_c_abi_argument_errors_without_a_gpu():
    import ctypes as C
    from nksr_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    A, Z = C.cast(buf, C.c_void_p), None

    def err():
        return lib.nksr_last_error().decode()

    assert lib.nksr_bnd_flags(A, A, 2, 3, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_flags(A, A, 1, 4, A, Z) != 0 and 'n_edges' in err()
    assert lib.nksr_bnd_flags(A, A, (1 << 30) + 1, 3, A, Z) != 0 and '2^30' in err()
    assert lib.nksr_bnd_list(A, 0, 2, A, A, 7, A, A, A, A, Z) != 0 and 'n_boundary' in err()
    assert lib.nksr_bnd_list(A, 0, 2, A, A, 3, A, Z, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_list(Z, 0, 0, Z, Z, 0, Z, Z, Z, Z, Z) == 0
    assert lib.nksr_bnd_successor(A, 0, 2, A, A, A, A, A, 3, A, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_successor(A, 0, -1, A, A, A, A, A, 3, A, A, Z) != 0 and 'negative' in err()
    assert lib.nksr_bnd_successor(Z, 0, 2, Z, Z, Z, Z, Z, 0, Z, Z, Z) == 0
    assert lib.nksr_bnd_loop_sizes(A, A, A, A, 4, A, 5, A, A, A, A, A, Z) != 0 and 'loops' in err()
    assert lib.nksr_bnd_loop_sizes(A, A, A, A, 4, A, 2, A, A, Z, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_loop_sizes(A, A, A, A, 1 << 31, A, 2, A, A, A, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_bnd_terms(A, 0, 3, A, A, A, A, A, A, 4, A, A, A, A, 2, A, A, A, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_terms(A, 0, 1 << 31, A, A, A, A, A, A, 4, A, A, A, A, 2, A, A, A, A, Z) != 0 and 'vertices' in err()
    assert lib.nksr_bnd_terms(Z, 0, 0, Z, Z, Z, Z, Z, Z, 0, Z, Z, Z, Z, 0, Z, Z, Z, Z, Z) == 0
    assert lib.nksr_bnd_boxes(A, 0, 3, A, A, A, 4, 2, Z, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_boxes(Z, 0, 0, Z, Z, Z, 0, 0, Z, Z, Z) == 0
    assert lib.nksr_bnd_fill(A, A, A, A, 4, A, A, A, A, A, 1, 2, 3, 4, A, 0, A, Z) != 0 and 'method' in err()
    assert lib.nksr_bnd_fill(A, A, A, A, 4, A, A, A, A, A, 1, 0, 3, 5, A, 0, A, Z) != 0 and 'new faces' in err()
    assert lib.nksr_bnd_fill(A, A, A, A, 4, A, A, A, A, A, 1, 0, (1 << 31) - 1, 4, A, 0, A, Z) != 0 and 'int32' in err()
    assert lib.nksr_bnd_fill(A, A, A, A, 4, A, A, A, A, A, 1, 1, 3, 2, Z, 0, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_fill(Z, Z, Z, Z, 0, Z, Z, Z, Z, Z, 0, 0, 0, 0, Z, 0, Z, Z) == 0
    assert lib.nksr_bnd_fill_vertices(A, A, A, A, A, A, 2, 3, Z, 0, 0, 3, A, 0, Z, Z) != 0 and 'kept' in err()
    assert lib.nksr_bnd_fill_vertices(A, A, A, A, A, A, 2, 1, Z, 0, 3, 3, A, 0, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_bnd_fill_vertices(Z, Z, Z, Z, Z, Z, 2, 0, Z, 0, 0, 3, Z, 0, Z, Z) == 0


def test_mesh_boundary_is_exported_and_documented():
    import nksr
    from nksr_amd import build, mesh_boundary, mesh_slice, mesh_topology
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_boundary import MeshBoundary
    assert 'MeshBoundary' in nksr.__all__ and nksr.MeshBoundary is MeshBoundary and nksr.metrics.MeshBoundary is MeshBoundary
    assert 'meshbound.hip' in build.SOURCES and callable(MeshingResult.boundary_loops) and callable(MeshingResult.fill_holes)
    assert isinstance(mesh_topology.MeshTopology.halfedge_edge, property) and callable(mesh_slice.halfedge_edges)
    doc = mesh_boundary.__doc__
    assert 'bit for bit' in doc and 'injective' in doc and 'fixed=~new_vertex_mask' in doc and 'threshold' in mesh_boundary.BoundaryLoops.select.__doc__
    assert callable(MeshBoundary.from_topology) and set(mesh_boundary.METHODS) == {'centroid', 'fan'}
