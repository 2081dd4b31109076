"""The numpy / scipy restatement of the mesh topology (tests/mesh_topology_ref.py) against hand-known answers, and the argument errors
of the C ABI of csrc/meshtopo.hip without a GPU."""
import numpy as np

import mesh_topology_ref as T


def test_restatement_on_closed_surfaces():
    for (v, f), chi in ((T.uv_sphere(64, 32), 2), (T.torus(96, 48), 0)):
        t = T.edge_table(f, len(v))
        assert (t['boundary_edges'], t['nonmanifold_edges'], t['misoriented_edges'], t['invalid_faces']) == (0, 0, 0, 0)
        assert t['num_edges'] == 3 * len(f) // 2 and t['euler'] == chi and t['referenced_vertices'] == len(v)
        assert (t['face_adjacency'] >= 0).all()
        for conn in ('edge', 'vertex'):
            c = T.components(v, f, conn)
            assert c['n'] == 1 and c['euler'].tolist() == [chi] and c['closed'].tolist() == [True]
            assert c['face_count'].tolist() == [len(f)] and c['vertex_count'].tolist() == [len(v)]
    v, f = T.uv_sphere(64, 32, 0.4)
    assert abs(T.components(v, f)['area'][0] / (4 * np.pi * 0.16) - 1) < 0.01


def test_restatement_on_the_hollow_shell():
    v, f = T.voxel_mesh(T.voxel_sets()['shell'], 0)
    for conn in ('edge', 'vertex'):
        c = T.components(v, f, conn)
        assert c['n'] == 2 and c['euler'].tolist() == [2, 2] and c['closed'].all()
        assert c['area'].tolist() == [150.0, 42.0]                      # the 5^3 block outside, the 3 x 3 x 2 cavity inside
        assert c['box'][0].tolist() == [0, 0, 0, 5, 5, 5] and c['box'][1].tolist() == [1, 1, 1, 4, 4, 3]
    assert T.edge_table(f, len(v))['euler'] == 4


def test_restatement_orientation_holes_and_fans():
    v, f = T.uv_sphere(64, 32)
    g = f.copy()
    g[100] = g[100][::-1]
    t = T.edge_table(g, len(v))
    assert t['misoriented_edges'] == 3 and t['boundary_edges'] == 0
    t = T.edge_table(np.delete(f, [200], 0), len(v))
    assert t['boundary_edges'] == 3 and t['euler'] == 1
    v, f = T.three_fan()
    t = T.edge_table(f, len(v))
    assert t['nonmanifold_edges'] == 1 and t['num_edges'] == 7 and t['boundary_edges'] == 6
    e = int(np.nonzero(t['edge_classes'] == T.NONMANIFOLD)[0][0])
    assert t['edges'][e].tolist() == [0, 1] and t['edge_counts'][e] == 3 and (t['face_adjacency'] == -1).all()
    assert T.components(v, f, 'edge')['n'] == 1


def test_restatement_components_and_compaction():
    v, f = T.two_cubes_sharing_a_vertex()
    assert len(v) == 15 and T.components(v, f, 'vertex')['n'] == 1
    c = T.components(v, f, 'edge')
    assert c['n'] == 2 and c['vertex_count'].tolist() == [8, 8] and c['euler'].tolist() == [2, 2]
    assert c['face_label'].tolist() == [0] * 12 + [1] * 12 and sorted(c['vertex_label'].tolist()) == [0] * 8 + [1] * 7
    # labels follow the minimum node index whatever the input order; an invalid face and an unreferenced vertex get -1
    v = np.zeros((9, 3), np.float32)
    f = np.array([[6, 7, 8], [0, 1, 2], [3, 3, 4], [2, 1, 9], [7, 6, 4]], np.int64)
    for conn, vl in (('edge', [1, 1, 1, -1, 0, -1, 0, 0, 0]), ('vertex', [0, 0, 0, -1, 1, -1, 1, 1, 1])):
        c = T.components(v, f, conn)
        assert c['n'] == 2 and c['vertex_label'].tolist() == vl
        assert c['face_label'].tolist() == ([0, 1, -1, -1, 0] if conn == 'edge' else [1, 0, -1, -1, 1])
    v2, f2, c2, vmap = T.compact(np.arange(27, dtype=np.float32).reshape(9, 3), f, [1, 0, 1, 1, 1], np.arange(9))
    assert f2.tolist() == [[1, 2, 3], [2, 1, 0]] and vmap.tolist() == [-1, -1, -1, -1, 0, -1, 1, 2, 3] and c2.tolist() == [4, 6, 7, 8]
    assert v2[:, 0].tolist() == [12, 18, 21, 24]
    v, f = T.uv_sphere(64, 32)
    v2, f2, _, vmap = T.compact(v, f, np.ones(len(f), bool))
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(vmap, np.arange(len(v)))


def test_topology_c_abi_argument_errors_without_a_gpu():
    """Argument validation happens before any launch: error code + message on a machine without a GPU, never an abort."""
    import ctypes as C
    from nksr_amd import _lib
    lib, null = _lib.lib, C.c_void_p(0)

    def err():
        return lib.nksr_last_error().decode()

    i64 = C.c_int64
    one = (C.c_int64 * 16)()
    big = i64((1 << 30) + 1)
    assert lib.nksr_topo_halfedge_keys(null, 0, i64(5), i64(9), null, null, null, null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_halfedge_keys(one, 0, i64(-1), i64(9), one, one, one, one, null) == _lib.ERR_ARG and 'negative' in err()
    assert lib.nksr_topo_halfedge_keys(one, 0, big, i64(9), one, one, one, one, null) == _lib.ERR_ARG and '2^30' in err()
    assert lib.nksr_topo_halfedge_keys(one, 0, i64(1), i64(1 << 31), one, one, one, one, null) == _lib.ERR_ARG and '2^31' in err()
    u64, every = C.c_uint64, C.c_uint64((1 << 64) - 1)
    assert lib.nksr_run_counts_u64(null, i64(6), every, null, null) == _lib.ERR_ARG and 'NULL' in err() and 'run counts' in err()
    assert lib.nksr_run_counts_u64(one, i64(-6), every, one, null) == _lib.ERR_ARG and 'negative' in err() and 'run counts' in err()
    assert lib.nksr_run_counts_u64(one, i64(1 << 32), every, one, null) == _lib.ERR_ARG and '2^32' in err() and 'run counts' in err()
    assert lib.nksr_run_table_u64(one, i64(6), u64(9), one, i64(7), one, one, one, null) == _lib.ERR_ARG and 'n_runs' in err() and 'run table' in err()
    assert lib.nksr_run_table_u64(one, i64(6), u64(9), one, i64(-1), one, one, one, null) == _lib.ERR_ARG and 'n_runs' in err()
    assert lib.nksr_run_table_u64(null, i64(6), u64(9), null, i64(2), null, null, null, null) == _lib.ERR_ARG and 'NULL' in err() and 'run table' in err()
    assert lib.nksr_run_table_u64(one, i64(-6), u64(9), one, i64(2), one, one, one, null) == _lib.ERR_ARG and 'negative' in err()
    assert lib.nksr_run_table_u64(one, i64(1 << 32), u64(9), one, i64(2), one, one, one, null) == _lib.ERR_ARG and '2^32' in err()
    assert lib.nksr_run_table_u64(one, i64((1 << 32) - 1), u64(9), one, i64(1 << 31), one, one, one, null) == _lib.ERR_ARG and '2^31' in err()
    assert lib.nksr_topo_face_pairs(one, one, i64(7), i64(9), one, null) == _lib.ERR_ARG and 'three times' in err()
    assert lib.nksr_topo_face_pairs(one, one, i64(3 * ((1 << 30) + 1)), i64(9), one, null) == _lib.ERR_ARG and '2^30' in err()
    assert lib.nksr_topo_edge_classes(null, 0, i64(2), i64(9), null, null, null, i64(3), null, null, null, null, null, null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_edge_classes(one, 0, big, i64(9), one, one, one, i64(3), one, one, one, one, one, one, null) == _lib.ERR_ARG and '2^30' in err()
    assert lib.nksr_topo_face_pairs(null, null, i64(6), i64(9), null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_uf_components(null, i64(4), null, null, i64(0), null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_uf_components(one, i64(-4), null, one, i64(1), one, null) == _lib.ERR_ARG and 'negative' in err()
    assert lib.nksr_uf_components(one, i64(1 << 31), null, one, i64(1), one, null) == _lib.ERR_ARG and 'int32' in err()
    assert lib.nksr_uf_labels(null, i64(4), null, null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_cross_labels(null, 0, i64(2), i64(9), null, 0, null, null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_component_counts(null, i64(2), null, i64(9), null, null, null, i64(3), i64(1), null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_component_counts(one, i64(2), one, i64(9), one, one, one, i64(3), i64(-1), one, null) == _lib.ERR_ARG and 'negative' in err()
    assert lib.nksr_topo_shared_corners(null, 0, i64(2), i64(9), null, null, null, i64(0), null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_count_shared(null, i64(2), i64(1), null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_component_boxes(null, i64(9), null, 0, i64(2), null, i64(1), null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_compact_mark(null, 0, i64(2), i64(9), null, null, null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_compact_faces(null, 0, i64(2), i64(9), null, null, null, null, null, null, null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_topo_compact_faces(one, 0, big, i64(9), one, one, one, one, one, one, null) == _lib.ERR_ARG and '2^30' in err()
    nbytes = C.c_size_t(0)
    assert lib.nksr_inclusive_sum_by_key_f64(one, C.byref(nbytes), null, null, null, i64(4), null) == _lib.ERR_ARG and 'NULL' in err()
    assert lib.nksr_inclusive_sum_by_key_f64(null, None, null, null, null, i64(4), null) == _lib.ERR_ARG and 'tmp_bytes' in err()
    assert lib.nksr_run_blocks(i64(0)) == 0 and lib.nksr_run_blocks(i64(257)) == 2
    import pytest
    with pytest.raises(RuntimeError):
        _lib.call('nksr_topo_face_pairs', null, null, 6, 9, null, null)
