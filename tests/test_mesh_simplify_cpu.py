"""The numpy restatement of the mesh simplification (tests/mesh_simplify_ref.py) against known answers -- it has to earn its place as the
yardstick of tests/test_gpu_mesh_simplify.py -- and the argument errors of the C ABI of csrc/meshsimp.hip, which need no GPU."""
import math

import numpy as np
import pytest

import mesh_simplify_ref as S
import mesh_topology_ref as T


@pytest.mark.parametrize('cell, faces', [(0.05, 1814), (0.1, 534), (0.2, 114)])
def test_the_sphere_stays_a_sphere(cell, faces):
    v, f = T.uv_sphere(64, 32)
    r = S.simplify(v, f, cell)
    assert len(r['f2']) == faces and r['duplicate_faces'] == 0
    assert r['collapsed_faces'] + faces == len(f) and r['invalid_faces'] == 0
    watertight, euler = S.closed_manifold_oriented(r['f2'], len(r['v2']))
    assert watertight and euler == 2
    assert r['v2'].dtype == v.dtype and r['f2'].dtype == f.dtype and r['vertex_map'].shape == (len(v),)
    assert r['f2'].max() == len(r['v2']) - 1 and (r['vertex_map'] >= 0).all()          # every cluster of a closed sphere keeps a face


def test_duplicate_faces_of_a_flattened_torus():
    v, f = T.torus(96, 48)
    assert S.count_faces(v, f, 0.3) == 10 and S.count_faces(v, f, 0.3, dedup=False) == 20
    r = S.simplify(v, f, 0.3)
    assert r['duplicate_faces'] == 10 and len(r['f2']) == 10
    kept = np.sort(r['f2'], axis=1)
    assert len(np.unique(kept, axis=0)) == 10


def test_quadrics_keep_the_corners_of_the_rotated_cube():
    v, f = S.rotated_cube()
    assert v.shape == (866, 3) and f.shape == (1728, 3) and v.dtype == np.float64
    q, m = S.simplify(v, f, 2.5), S.simplify(v, f, 2.5, placement='mean')
    assert q['n_clusters'] == 160 and len(q['f2']) == 318 and np.array_equal(q['f2'], m['f2'])
    cq, cm = S.corner_error(q['v2']), S.corner_error(m['v2'])
    pq, pm = S.plane_error(q['v2']), S.plane_error(m['v2'])
    print('corner distance: quadric %.3e, mean %.3e; plane distance: quadric %.3e, mean %.3e' % (cq, cm, pq, pm))
    assert 10 * cq <= cm and cm > 1.0
    assert pq < 0.1 and pm > 0.6 and 6 * pq <= pm
    # every representative lies in the closed box of its cell (to the rounding of centre + x at coordinates of ~ 16)
    keys = S.clusters(v, f, 2.5)[2]
    cells = np.stack([keys >> 42, (keys >> 21) & (S.MAX_INDEX - 1), keys & (S.MAX_INDEX - 1)], 1)
    for r in (q, m):
        local = (r['representatives'] - r['origin']) / 2.5
        assert (np.abs(local - (cells + 0.5)) <= 0.5 + 1e-14).all()


def test_the_cube_does_not_move_at_an_offset_of_a_million():
    v, f = S.rotated_cube()
    near, far = S.simplify(v, f, 2.5), S.simplify(S.rotated_cube(1e6)[0], f, 2.5)
    # the shifted vertices round at 1e6 2^-53 = 1.1e-10, which may move one across a cell face: the clusters are compared, not assumed
    assert np.array_equal(near['cluster_id'], far['cluster_id']) and np.array_equal(near['f2'], far['f2'])
    d = float(np.abs(far['v2'] - 1e6 - near['v2']).max())
    print('max |v2(1e6) - 1e6 - v2| = %.3e' % d)
    assert d <= 1e-8 and abs(S.corner_error(far['v2'], 1e6) - S.corner_error(near['v2'])) <= 1e-8


def test_a_cell_below_the_vertex_spacing_returns_the_compacted_input():
    v, f, col, _ = T.sphere_with_floaters()
    v = np.concatenate([v, [[5.0, 5.0, 5.0]]]).astype(np.float32)                 # an unreferenced vertex
    f = np.concatenate([f, [[0, 0, 1], [0, 1, len(v) + 3]]])                      # two invalid faces
    col = np.concatenate([col, [[0.5, 0.5, 0.5]]]).astype(np.float32)
    cell = 1e-4
    r = S.simplify(v, f, cell, colors=col)
    v2, f2, c2, vmap = T.compact(v, f, np.ones(len(f), bool), col)
    assert r['n_clusters'] == len(v2) and r['invalid_faces'] == 2 and r['collapsed_faces'] == 0 and r['duplicate_faces'] == 0
    order = r['cluster_id'][vmap >= 0]                                             # compacted vertex i became cluster order[i]
    assert np.array_equal(np.sort(order), np.arange(len(v2)))
    assert np.abs(r['v2_f64'][order] - v2.astype(np.float64)).max() <= 1e-12 * cell
    assert np.array_equal(r['c2'][order], c2) and np.array_equal(r['f2'], order[f2])
    assert np.array_equal(r['vertex_map'][vmap >= 0], order) and (r['vertex_map'][vmap < 0] == -1).all()
    keys = S.clusters(v, f, cell)[2]
    assert (np.diff(keys) > 0).all()


def test_grid_errors_and_the_caller_origin():
    v = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [2097151.25, 0, 0], [2097151.5, 0.5, 0], [2097151.75, 0, 0.5]], np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    r = S.simplify(v, f, 1.0)                                                      # the far triangle at index 2^21 - 1: one cluster
    assert r['n_clusters'] == 2 and len(r['f2']) == 0 and r['collapsed_faces'] == 2
    with pytest.raises(ValueError):
        S.simplify(v + np.array([[0, 0, 0]] * 3 + [[0.75, 0, 0]] * 3), f, 1.0)    # ... at index 2^21
    with pytest.raises(ValueError):
        S.simplify(v, f, 1.0, origin=[0.0, 1e-9, 0.0])
    sv, sf = T.uv_sphere(64, 32)
    a, b = S.simplify(sv, sf, 0.1), S.simplify(sv, sf, 0.1, origin=[-0.43, -0.47, -0.41])
    assert len(a['f2']) != len(b['f2']) or not np.array_equal(a['v2'], b['v2'])   # the grid moved
    with pytest.raises(ValueError):
        S.simplify(np.array([[0, 0, 0], [1, 0, 0], [0, np.nan, 0]]), np.array([[0, 1, 2]]), 1.0)
    ok = S.simplify(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]]), np.array([[0, 1, 2]]), 0.3)     # unreferenced: ignored
    assert len(ok['f2']) == 1 and ok['vertex_map'][3] == -1


def test_the_target_search_takes_24_steps_and_stays_below_the_target():
    v, f = T.uv_sphere(64, 32)
    diag = S.diagonal(v, f)
    assert abs(diag - 0.8 * math.sqrt(3)) < 1e-2
    calls = []

    def count(h):
        calls.append(h)
        return S.count_faces(v, f, h)
    for target in (3000, 500, 50, 0):
        del calls[:]
        h, steps = S.target_cell_size(count, diag, target)
        assert steps == 24 and len(calls) == 25 and S.count_faces(v, f, h) <= target
        assert diag / 2.0 ** 20 < h <= 2.0 * diag
    assert S.target_cell_size(count, diag, len(f)) == (diag / 2.0 ** 20, 0)
    assert S.count_faces(v, f, 2.0 * diag) == 0                                    # hi: one cluster, whatever the origin


def test_simplify_c_abi_argument_errors_without_a_gpu():
    """Argument validation happens before anything is launched or cleared: error code + message without a GPU, never an abort."""
    import ctypes as C
    from nksr_amd import _lib
    lib, null = _lib.lib, C.c_void_p(0)

    def err():
        return lib.nksr_last_error().decode()

    i64, dbl = C.c_int64, C.c_double
    one = (C.c_int64 * 16)()
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    bad3 = (C.c_double * 3)(0.0, float('inf'), 0.0)
    big, E = i64((1 << 30) + 1), _lib.ERR_ARG
    assert lib.nksr_simp_cell_keys(null, 0, i64(5), null, o3, dbl(1.0), null, null, one, null) == E and 'NULL' in err()
    assert lib.nksr_simp_cell_keys(one, 0, i64(5), one, o3, dbl(1.0), one, one, null, null) == E and 'NULL' in err()
    assert lib.nksr_simp_cell_keys(one, 0, i64(5), one, null, dbl(1.0), one, one, one, null) == E and 'origin' in err()
    assert lib.nksr_simp_cell_keys(one, 0, i64(5), one, bad3, dbl(1.0), one, one, one, null) == E and 'origin' in err()
    for h in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.nksr_simp_cell_keys(one, 0, i64(5), one, o3, dbl(h), one, one, one, null) == E and 'cell_size' in err(), h
    assert lib.nksr_simp_cell_keys(one, 0, i64(1 << 31), one, o3, dbl(1.0), one, one, one, null) == E and '2^31' in err()
    every = C.c_uint64((1 << 64) - 1)                                              # the clusters are the run table of the sorted keys
    assert lib.nksr_run_counts_u64(null, i64(5), every, one, null) == E and 'NULL' in err()
    assert lib.nksr_run_counts_u64(one, i64(-5), every, one, null) == E and 'negative' in err()
    assert lib.nksr_run_table_u64(one, i64(5), every, one, i64(6), one, one, one, null) == E and 'n_runs' in err()
    assert lib.nksr_run_table_u64(one, i64(5), every, one, i64(2), null, one, one, null) == E and 'NULL' in err()
    assert lib.nksr_simp_face_remap(null, 0, i64(5), i64(9), one, one, one, one, one, one, one, one, null) == E and 'NULL' in err()
    assert lib.nksr_simp_face_remap(one, 0, big, i64(9), one, one, one, one, one, one, one, one, null) == E and '2^30' in err()
    assert lib.nksr_simp_flag_duplicates(null, i64(5), one, one, one, one, one, null) == E and 'NULL' in err()
    assert lib.nksr_simp_flag_duplicates(one, i64(5), one, one, one, one, null, null) == E and 'NULL' in err()
    args = [one, 0, i64(9), one, 0, i64(5), one, one, one, one, one, i64(4), o3, dbl(0.5), dbl(1e-3), _lib.SIMP_QUADRIC, one, null]
    for k in (0, 3, 6, 7, 8, 9, 10, 16):
        bad = list(args)
        bad[k] = null
        assert lib.nksr_simp_place(*bad) == E and 'NULL' in err(), k
    for k, value, word in ((15, 2, 'placement'), (14, dbl(0.0), 'regularisation'), (14, dbl(1.5), 'regularisation'), (14, dbl(float('nan')), 'regularisation'),
                           (13, dbl(0.0), 'cell_size'), (11, i64(10), 'n_clusters'), (5, big, '2^30'), (12, null, 'origin')):
        bad = list(args)
        bad[k] = value
        assert lib.nksr_simp_place(*bad) == E and word in err(), (k, err())
    mean = list(args)
    mean[11] = i64(0)                                                              # no cluster: nothing is launched
    assert lib.nksr_simp_place(*mean) == 0
    assert lib.nksr_simp_cluster_means(null, 0, i64(9), i64(3), one, one, i64(4), one, null) == E and 'NULL' in err()
    assert lib.nksr_simp_cluster_means(one, 0, i64(9), i64(-3), one, one, i64(4), one, null) == E and 'channels' in err()
    assert lib.nksr_simp_cluster_means(one, 0, i64(9), i64(3), one, one, i64(0), one, null) == 0


def test_exports_and_the_build_flags():
    import nksr
    from nksr_amd import _lib, build
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_simplify import MeshSimplifier
    assert 'MeshSimplifier' in nksr.__all__ and nksr.MeshSimplifier is MeshSimplifier and nksr.metrics.MeshSimplifier is MeshSimplifier
    assert 'meshsimp.hip' in build.SOURCES and callable(MeshingResult.simplify)
    assert _lib.SIMP_MAX_INDEX == 1 << 21 == S.MAX_INDEX and _lib.SIMP_GROUP == 16
    # the cell index is an fp64 division: no flag of the build may let the compiler turn it into a product with a reciprocal
    assert not any('fast' in flag or 'recip' in flag or 'unsafe' in flag for flag in build.FLAGS)
    assert 'bit for bit' in __import__('nksr_amd.mesh_simplify').mesh_simplify.__doc__
