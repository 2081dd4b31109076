"""Mesh queries without a GPU: the numpy restatement of the crossing predicate (tests/mesh_query_ref.py, the kernel's arithmetic in
csrc/meshquery.hip) against exact truth, and the C-ABI's argument checks before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_query_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _voxel_cases():
    return {k: R.voxel_mesh(s, diag_seed=i) + (s,) for i, (k, s) in enumerate(sorted(R.voxel_sets().items()))}


@pytest.mark.parametrize('kind', ['blob', 'pocket', 'shell', 'stairs'])
def test_restatement_is_exact_on_voxel_unions(kind):
    """rays = 1: the parity of ONE ray is the exact inside at every lattice point off the surface, although many of these rays run
    exactly through shared edges and vertices; so is every other ray of the table."""
    from parity_util import assert_closed
    v, f, vox = _voxel_cases()[kind]
    assert_closed(f, kind)
    q, inside = R.voxel_queries(vox, v, f)
    v32, q32 = R.recentre(v, q)
    counts = R.crossings(v32, f, q32, R.DIRS.shape[0])
    for r in range(counts.shape[1]):
        assert np.array_equal(counts[:, r] % 2 == 1, inside), (kind, r, int(((counts[:, r] % 2 == 1) != inside).sum()))
    assert np.array_equal(R.occupancy_from_counts(counts[:, :1]), inside)
    assert np.array_equal(R.occupancy_from_counts(counts[:, :3]), inside)
    assert inside.sum() > 50 and (~inside).sum() > 500
    # the same counts with every face flipped: the predicate does not read the orientation
    flipped = R.crossings(v32, f[:, ::-1], q32, 3)
    assert np.array_equal(flipped, counts[:, :3])


def test_voxel_rays_meet_edges_and_vertices_exactly():
    """The lattice rays hit shared edges and vertices exactly (edge functions that are 0 in the sheared frame): a test that counts
    a zero as a hit, or as a miss, on both triangles of an edge gets these queries wrong."""
    v, f, vox = _voxel_cases()['pocket']
    q, inside = R.voxel_queries(vox, v, f)
    v32, q32 = R.recentre(v, q)
    zeros, wrong_incl, wrong_excl = 0, 0, 0
    d = R.DIRS[0]
    kx, ky, kz, sx, sy, _ = R._frame(d)
    for o, truth in zip(q32, inside):
        x = v32 - o[None]
        px, py = x[:, kx] - sx * x[:, kz], x[:, ky] - sy * x[:, kz]
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        e = [px[b] * py[c] - py[b] * px[c], px[c] * py[a] - py[c] * px[a], px[a] * py[b] - py[a] * px[b]]
        zeros += int(sum((x_ == 0).sum() for x_ in e))
        z = x[:, kz] * d[kz]
        T = e[0] * z[a] + e[1] * z[b] + e[2] * z[c]
        det = e[0] + e[1] + e[2]
        for incl in (True, False):
            pos = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) if incl else (e[0] > 0) & (e[1] > 0) & (e[2] > 0)
            neg = (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0) if incl else (e[0] < 0) & (e[1] < 0) & (e[2] < 0)
            hit = (pos & (det > 0) & (T > 0)) | (neg & (det < 0) & (T < 0))
            wrong = (int(hit.sum()) % 2 == 1) != truth
            wrong_incl += wrong if incl else 0
            wrong_excl += wrong if not incl else 0
    assert zeros > 100
    assert wrong_incl > 0 and wrong_excl > 0


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_is_exact_on_convex_polyhedra(seed):
    v, f, nrm, off = R.convex_polyhedron(30 + 10 * seed, seed)
    rs = np.random.RandomState(seed)
    q = rs.uniform(-1.2, 1.2, (3000, 3))
    inside, gap = R.inside_halfspaces(nrm, off, q)
    keep = gap > 1e-6
    q, inside = q[keep], inside[keep]
    v32, q32 = R.recentre(v, q)
    # (the truth is taken of the float32 points the kernel sees)
    c = 0.5 * (v.astype(np.float64).min(0) + v.astype(np.float64).max(0))
    inside = R.inside_halfspaces(nrm, off, q32.astype(np.float64) + c)[0]
    counts = R.crossings(v32, f, q32, 3)
    assert np.array_equal(R.occupancy_from_counts(counts[:, :1]), inside)
    assert np.array_equal(R.occupancy_from_counts(counts), inside)
    assert (counts[inside] == 1).all() and counts.max() <= 2 and inside.sum() > 100     # a convex body: a half-line meets it twice at most


def test_fp64_truths_agree_on_a_closed_mesh():
    """The winding number and the distance brute force used as truth by the GPU tests: |w| is 1 inside, 0 outside a closed sphere."""
    v, f = R.uv_sphere(24, 12, 0.4)
    rs = np.random.RandomState(0)
    q = rs.uniform(-0.6, 0.6, (400, 3))
    d, _ = R.distance_bruteforce(v, f, q)
    far = d > 1e-3
    w = R.winding_number(v, f, q[far])
    assert np.all(np.minimum(np.abs(w), np.abs(np.abs(w) - 1)) < 1e-9)
    v32, q32 = R.recentre(v, q[far])
    assert np.array_equal(R.occupancy_from_counts(R.crossings(v32, f, q32, 3)), np.abs(w) > 0.5)
    d2, face2 = R.distance_bruteforce(v, f, q, upper=d, margin=1e-9)
    assert np.array_equal(d2, d)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _err():
    from nksr_amd import _lib
    return _lib.lib.nksr_last_error().decode()


def test_header_constants_match_the_bindings():
    from nksr_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'nksr_hip.h')).read()
    m = re.search(r'#define NKSR_BVH_RAY_DIRS (.*?)\n(?!\s+\{)', src, flags=re.S)
    dirs = [float(x) for x in re.findall(r'(-?\d+\.\d+)f', m.group(1))]
    assert np.array_equal(np.array(dirs, np.float32).reshape(-1, 3), R.DIRS)
    assert np.array_equal(np.array(_lib.BVH_RAY_DIRS, np.float32), R.DIRS)
    for name, val in (('NODE_FLOATS', _lib.BVH_NODE_FLOATS), ('LEAF_FLOATS', _lib.BVH_LEAF_FLOATS), ('STACK', _lib.BVH_STACK),
                      ('MAX_RAYS', _lib.BVH_MAX_RAYS)):
        assert int(re.search(r'#define NKSR_BVH_%s (\d+)' % name, src).group(1)) == val
    assert C.sizeof(_lib.BvhT) == 8 + 8 + 4 * 8
    assert (np.abs(R.DIRS).max(1) == 1).all() and (R.DIRS != 0).all() and (np.sort(np.abs(R.DIRS), 1)[:, 1] < 1).all()


def test_mesh_query_entry_points_reject_bad_arguments():
    from nksr_amd import _lib
    lib = _lib.lib
    null = C.c_void_p(0)
    buf = (C.c_float * 64)()
    bvh = _lib.BvhT(1, 0, 0, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p))
    ARG, CAP = -1, -3
    # Morton codes: negative sizes, NULL arrays, more than 2^30 faces
    assert lib.nksr_bvh_morton(buf, C.c_int64(-1), buf, 0, C.c_int64(1), buf, buf, buf, null) == ARG and 'negative' in _err()
    assert lib.nksr_bvh_morton(buf, C.c_int64(3), buf, 0, C.c_int64(-1), buf, buf, buf, null) == ARG and 'negative' in _err()
    assert lib.nksr_bvh_morton(null, C.c_int64(3), buf, 0, C.c_int64(1), buf, buf, buf, null) == ARG and 'NULL' in _err()
    assert lib.nksr_bvh_morton(buf, C.c_int64(3), buf, 0, C.c_int64(1), null, buf, buf, null) == ARG and 'NULL' in _err()
    assert lib.nksr_bvh_morton(buf, C.c_int64(3), buf, 0, C.c_int64((1 << 30) + 1), buf, buf, buf, null) == ARG and '2^30' in _err()
    assert lib.nksr_bvh_morton(buf, C.c_int64(3), None, 0, C.c_int64(4), buf, buf, buf, null) == ARG and 'points' in _err()
    # nodes / refit: bad struct, NULL arrays
    assert lib.nksr_bvh_nodes(buf, buf, None, null) == ARG and 'NULL bvh' in _err()
    big = _lib.BvhT((1 << 30) + 1, 0, 0, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), None)
    assert lib.nksr_bvh_nodes(buf, buf, C.byref(big), null) == ARG and '2^30' in _err()
    neg = _lib.BvhT(-2, 0, 0, None, None, None, None)
    assert lib.nksr_bvh_nodes(buf, buf, C.byref(neg), null) == ARG
    two = _lib.BvhT(2, 0, 0, None, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p))
    assert lib.nksr_bvh_nodes(buf, buf, C.byref(two), null) == ARG and 'NULL' in _err()
    assert lib.nksr_bvh_refit(buf, C.c_int64(-3), buf, 0, buf, buf, buf, C.byref(bvh), null) == ARG and 'negative' in _err()
    assert lib.nksr_bvh_refit(buf, C.c_int64(3), buf, 0, None, buf, buf, C.byref(bvh), null) == ARG and 'NULL' in _err()
    assert lib.nksr_bvh_refit(buf, C.c_int64(0), buf, 0, buf, buf, buf, C.byref(bvh), null) == ARG and 'zero vertices' in _err()
    # queries: rays outside the table or even, negative sizes, NULL query / outputs, a tree deeper than the stack
    for rays in (0, 2, 4, 6, 8, 9, -1):
        assert lib.nksr_mesh_occupancy(C.byref(bvh), buf, C.c_int64(4), None, rays, buf, None, null) == ARG and 'rays' in _err()
    assert lib.nksr_mesh_occupancy(C.byref(bvh), buf, C.c_int64(-4), None, 3, buf, None, null) == ARG and 'negative' in _err()
    assert lib.nksr_mesh_occupancy(C.byref(bvh), None, C.c_int64(4), None, 3, buf, None, null) == ARG and 'NULL' in _err()
    assert lib.nksr_mesh_occupancy(C.byref(bvh), buf, C.c_int64(4), None, 3, None, None, null) == ARG and 'NULL' in _err()
    assert lib.nksr_mesh_occupancy(C.byref(big), buf, C.c_int64(4), None, 3, buf, None, null) == ARG
    assert lib.nksr_mesh_closest(C.byref(bvh), buf, C.c_int64(4), None, None, None, None, null) == ARG and 'no output' in _err()
    assert lib.nksr_mesh_closest(C.byref(bvh), buf, C.c_int64(-1), None, buf, None, None, null) == ARG and 'negative' in _err()
    assert lib.nksr_mesh_closest(None, buf, C.c_int64(4), None, buf, None, None, null) == ARG and 'NULL bvh' in _err()
    deep = _lib.BvhT(1, _lib.BVH_STACK + 1, 0, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), None)
    assert lib.nksr_mesh_closest(C.byref(deep), buf, C.c_int64(4), None, buf, None, None, null) == CAP and 'depth' in _err()
    assert lib.nksr_mesh_occupancy(C.byref(deep), buf, C.c_int64(4), None, 3, buf, None, null) == CAP and 'depth' in _err()
    # nothing to do is no error
    assert lib.nksr_mesh_occupancy(C.byref(bvh), buf, C.c_int64(0), None, 3, None, None, null) == 0
    with pytest.raises(RuntimeError):
        _lib.call('nksr_mesh_occupancy', C.byref(bvh), None, 4, None, 2, None, None, None)


def test_mesh_query_api_surface_and_ray_checks():
    import inspect
    import nksr
    from nksr.metrics import MeshEvaluator, MeshQuery, mesh_occupancy
    from nksr_amd import mesh_query
    assert nksr.metrics.MeshQuery is mesh_query.MeshQuery is MeshQuery
    assert list(inspect.signature(MeshQuery.__init__).parameters)[1:] == ['v', 'f', 'device']
    assert inspect.signature(MeshQuery.occupancy).parameters['rays'].default == 3
    assert list(inspect.signature(MeshQuery.distance).parameters)[1:] == ['points', 'closest_point']
    assert 'o3d-iou' not in MeshEvaluator.ALL_METRICS and 'o3d-iou' not in MeshEvaluator.ESSENTIAL_METRICS
    v, f = R.uv_sphere(8, 4)
    for rays in (0, 2, 4, 8, 1.0, True, '3'):
        with pytest.raises(ValueError):
            mesh_occupancy(v, f, np.zeros((2, 3)), rays=rays)
    with pytest.raises(RuntimeError):
        MeshQuery(v, f, device='cpu')
