"""The numpy restatement of the mesh clipper (tests/mesh_clip_ref.py) against hand-checked cases -- it has to earn its place as the
yardstick of tests/test_gpu_mesh_clip.py -- and the argument errors of the C ABI of csrc/meshclip.hip, which need no GPU."""
import numpy as np

import mesh_clip_ref as R

EPS = np.finfo(np.float64).eps


def _split(v, f, normal, offsets, attr=None):
    n = R.unit(normal)
    return R.split_mesh(v, f, n, offsets, R.heights(v, n), attr=attr)


def check_invariants(v, f, r, label=''):
    """2 k + 1 triangles per valid face, no flipped triangle, areas conserved per face under ``mesh_clip_ref.area_bound``."""
    v64 = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    slab = r['slab']
    for i in range(len(f)):
        n = r['face_start'][i + 1] - r['face_start'][i]
        if n:
            s = slab[f[i]]
            assert n == 2 * (s.max() - s.min()) + 1
    a2, n2 = R.face_areas(r['v2_64'], r['f2'])
    a0, n0 = R.face_areas(v64, f)
    dots = (n2 * n0[r['face_source']]).sum(1)
    scale = np.sqrt((n2 * n2).sum(1) * (n0 * n0).sum(1)[r['face_source']])
    assert np.all(dots >= -64 * EPS * np.maximum(scale, 1e-300)), (label, dots.min())      # never flipped (a zero-area triangle: rounding only)
    per_face = np.bincount(r['face_source'], weights=a2, minlength=len(f))
    valid = np.diff(r['face_start']) > 0
    err = np.abs(per_face - a0)[valid]
    bound = R.area_bound(v, f, r)[valid]
    print('%s: area error %.3g of bound %.3g' % (label, err.max(initial=0), bound.max(initial=0)))
    assert np.all(err <= bound)
    return a2


def test_cube_split_at_half_height():
    v, f = R.cube()
    r = _split(v, f, (0, 0, 1), [0.5])
    assert r['n_points'] == 8 and r['n_faces'] == 2 * 1 + 2 * 1 + 8 * 3 and r['n_parts'] == 2 and r['n_dropped'] == 0 and r['n_degenerate'] == 0
    assert np.array_equal(r['v2_64'][:8], v.astype(np.float64)) and np.all(r['v2_64'][8:, 2] == 0.5)
    a = check_invariants(v, f, r, 'cube')
    assert a[r['face_part'] == 0].sum() == 3.0 and a[r['face_part'] == 1].sum() == 3.0          # (dyadic: exact)
    assert np.array_equal(np.diff(r['face_start']), [1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 3])
    assert np.array_equal(r['face_source'], np.repeat(np.arange(12), np.diff(r['face_start'])))
    # two planes at the vertex heights: nothing is cut, the bottom faces are part 1 (on the plane counts as above), the top ones part 2
    r = _split(v, f, (0, 0, 1), [0.0, 1.0])
    assert r['n_points'] == 8 and r['n_faces'] == 4 + 8 * 3 and r['n_degenerate'] == 8 * 2
    assert set(r['face_part'][r['face_source'] < 2]) == {1} and set(r['face_part'][(r['face_source'] >= 2) & (r['face_source'] < 4)]) == {2}
    check_invariants(v, f, r, 'cube at its vertex heights')
    # no planes: the faces unchanged
    r = _split(v, f, (0, 0, 1), [])
    assert r['n_points'] == 0 and np.array_equal(r['f2'], f) and np.all(r['face_part'] == 0)


def test_first_piece_is_fanned_from_the_first_corner():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float64)
    f = np.array([[0, 1, 2]])
    r = _split(v, f, (1, 0, 0), [1.0, 3.0])
    # walk: c0 (slab 0), p(0|e01) = 3, p(1|e01) = 4, c1 (slab 2), p(1|e12) = 6, p(0|e12) = 5, c2 (slab 0): edges sorted (0,1), (0,2), (1,2)
    assert np.array_equal(r['point_edge'], [0, 0, 2, 2]) and np.array_equal(r['point_plane'], [0, 1, 0, 1])
    assert r['f2'].tolist() == [[0, 3, 5], [0, 5, 2], [3, 4, 6], [3, 6, 5], [4, 1, 6]]
    assert r['face_part'].tolist() == [0, 0, 1, 1, 2] and r['face_source'].tolist() == [0] * 5
    check_invariants(v, f, r, 'one triangle')
    r = _split(v, f[:, [1, 2, 0]], (1, 0, 0), [1.0, 3.0])                      # the same face starting at c1: other fans, same pieces
    assert r['f2'].tolist() == [[5, 2, 0], [5, 0, 3], [6, 5, 3], [6, 3, 4], [1, 6, 4]]


def test_tetrahedron_planes_through_a_vertex_an_edge_and_a_face():
    v, f = R.tetrahedron()
    r = _split(v, f, (0, 0, 1), [0.0])                                         # in the face z = 0: its vertices are ABOVE, nothing crosses
    assert r['n_points'] == 0 and r['n_faces'] == 4 and np.all(r['face_part'] == 1)
    r = _split(v, f, (0, 0, 1), [1.0])                                         # through the apex: three collapsed pieces
    assert r['n_points'] == 3 and r['n_faces'] == 1 + 3 * 3
    assert r['n_degenerate'] == 6                # per side face: the quad's second triangle and the collapsed piece above the plane
    assert np.all(r['v2_64'][4:] == v[3]) and np.count_nonzero(r['face_part'] == 1) == 3
    a = check_invariants(v, f, r, 'apex')
    assert np.all(a[r['face_part'] == 1] == 0.0)
    n = R.unit((1, 1, 0))
    h = R.heights(v, n)
    assert h[1] == h[2]
    r = R.split_mesh(v, f, n, [h[1]], h)                                       # through the edge (1, 2)
    assert r['n_points'] == 4 and r['point_edge'].tolist() == [0, 1, 4, 5]     # on the edges (0, 1), (0, 2), (1, 3), (2, 3), at the ends 1 and 2
    assert np.all(np.isin(r['v2_64'][4:], v[[1, 2]]).all(1)) and r['n_faces'] == 4 * 3 and r['n_degenerate'] == 4 * 2       # (two per face)
    check_invariants(v, f, r, 'edge')
    r = _split(v, f, (0, 0, 1), [-1.0, 0.25, 0.5, 2.0])
    assert r['n_parts'] == 5 and set(r['face_part']) == {1, 2, 3}
    check_invariants(v, f, r, 'two cuts')


def test_count_orientation_and_area_on_random_triangles():
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(300):
        integer = trial % 2 == 0
        v = rng.integers(-4, 5, (3, 3)).astype(np.float64) if integer else rng.normal(size=(3, 3))
        if np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])) == 0:
            continue
        axis = int(rng.integers(0, 3))
        n = R.axis_normal(axis) if integer else R.unit(rng.normal(size=3))
        k = int(rng.integers(0, 12))
        off = np.unique(rng.integers(-5, 6, k).astype(np.float64)) if integer else np.unique(rng.uniform(-2, 2, k))
        f = np.array([[0, 1, 2]])
        r = R.split_mesh(v, f, n, off, R.heights(v, n))
        a = check_invariants(v, f, r, 'random %d' % trial)
        a0 = R.face_areas(v, f)[0][0]
        worst = max(worst, abs(a.sum() - a0) / a0)
    print('worst relative area error %.3g' % worst)
    assert worst < 1e-12            # (a sanity check on well-conditioned triangles, far above the 4e-15 they measure)


def test_invalid_faces_are_dropped_and_attributes_interpolated():
    v, f = R.cube()
    f = np.concatenate([f, [[0, 0, 1], [0, 1, 99]]])
    attr = np.concatenate([v.astype(np.float64) * 2.0, np.ones((8, 1))], 1)
    r = _split(v, f, (0, 0, 1), [0.25], attr=attr)
    assert r['n_dropped'] == 2 and r['face_start'][-1] == r['face_start'][-3] == r['n_faces']
    assert np.array_equal(r['attr2_64'][:, :3], r['v2_64'] * 2.0) and np.all(r['attr2_64'][:, 3] == 1.0)


def test_grouping_numbers_vertices_label_major():
    v, f = R.cube()
    r = _split(v, f, (0, 0, 1), [0.5])
    g = R.group(r['f2'], r['face_part'], 2)
    assert g['part_vertex_start'].tolist() == [0, 12, 24] and g['part_face_start'].tolist() == [0, 14, 28]
    assert g['vertex_source'].tolist() == [0, 1, 2, 3] + list(range(8, 16)) + [4, 5, 6, 7] + list(range(8, 16))
    for j in range(2):
        pv, pf, _ = R.part_mesh(g, j, r['v2_64'])
        assert pf.min() == 0 and pf.max() == 11 and R.face_areas(pv, pf)[0].sum() == 3.0
    lab = np.where(np.arange(28) % 2 == 0, 3, 1)                               # labels 0 and 2 stay empty
    g = R.group(r['f2'], lab, 5)
    assert g['part_face_start'].tolist() == [0, 0, 14, 14, 28, 28] and np.array_equal(g['face_order'][:14], np.arange(1, 28, 2))
    assert np.array_equal(r['f2'][g['face_order']], g['vertex_source'][g['f']])
    bv, bf, _ = R.clip_box(*R.cube(lo=(-1, -1, -1), size=(2, 2, 2)), (0, 0, 0), (4, 4, 4))
    assert bv.min() == 0.0 and bv.max() == 1.0 and R.face_areas(bv, bf)[0].sum() == 3.0


def test_clip_c_abi_argument_errors_without_a_gpu():
    import ctypes as C
    from nksr_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    A, Z = C.cast(buf, C.c_void_p), None

    def err():
        return lib.nksr_last_error().decode()

    assert lib.nksr_clip_faces(A, 3, A, 0, 1, A, A, A, 0, A, 1, A, A, 1, 1, 0, Z, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_clip_faces(A, 3, A, 0, 1, A, A, A, 0, A, 1, A, Z, 1, 1, 1, A, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_clip_faces(A, 3, A, 0, -1, A, A, A, 0, A, 1, A, A, 1, 1, 0, A, A, A, Z) != 0 and 'negative' in err()
    assert lib.nksr_clip_faces(A, 3, A, 0, 1, A, A, A, 0, A, 1, A, A, 1, 1 << 31, 0, A, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_clip_faces(A, 3, A, 0, 1, A, A, A, (1 << 31) - 3, A, 1, A, A, 1, 1, 0, A, A, A, Z) != 0 and 'points' in err()
    assert lib.nksr_clip_faces(A, 3, A, 0, 1, A, A, A, 2, A, 1, A, A, 1, 4, 0, A, A, A, Z) != 0 and 'pieces' in err()
    assert lib.nksr_clip_faces(A, 3, A, 0, 0, A, A, A, 0, A, 1, A, A, 1, 1, 0, A, A, A, Z) != 0 and 'without faces' in err()
    assert lib.nksr_clip_faces(Z, 0, Z, 0, 0, Z, Z, Z, 0, Z, 0, Z, Z, 0, 0, 0, Z, Z, Z, Z) == 0
    assert lib.nksr_clip_attr(A, 0, 3, 2, A, A, 3, A, 1, A, A, 2, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_clip_attr(A, 0, 3, -1, A, A, 3, A, 1, A, A, 2, A, Z) != 0 and 'channels' in err()
    assert lib.nksr_clip_attr(A, 0, 3, 2, A, A, 0, A, 1, A, A, 2, A, Z) != 0 and 'without edges' in err()
    assert lib.nksr_clip_attr(Z, 0, 0, 2, Z, Z, 0, Z, 0, Z, Z, 0, Z, Z) == 0
    assert lib.nksr_clip_corner_keys(A, Z, 2, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_clip_corner_keys(A, A, -1, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_clip_corner_keys(A, A, (1 << 31) // 3 + 1, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_clip_corner_keys(Z, Z, 0, Z, Z, Z) == 0
    assert lib.nksr_clip_group_faces(A, A, 2, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_clip_group_faces(A, A, -2, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_clip_group_faces(Z, Z, 0, Z, Z) == 0


def test_mesh_clipper_is_exported_and_documented():
    import nksr
    from nksr_amd import build, mesh_clip
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_clip import MeshClipper
    assert 'MeshClipper' in nksr.__all__ and nksr.MeshClipper is MeshClipper and nksr.metrics.MeshClipper is MeshClipper
    assert 'meshclip.hip' in build.SOURCES
    assert all(callable(getattr(MeshingResult, name)) for name in ('split', 'clip', 'clip_box', 'tiles'))
    assert all(callable(getattr(MeshClipper, name)) for name in ('split', 'clip', 'clip_box', 'tiles', 'from_topology'))
    assert 'bit for bit' in mesh_clip.__doc__ and '2 k + 1' in mesh_clip.__doc__ and mesh_clip.FACES_BY_PIECE in (0, 1)
    assert 'fill_holes' in MeshClipper.clip.__doc__
