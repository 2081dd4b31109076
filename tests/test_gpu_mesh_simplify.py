"""Mesh simplification on the MI355X (nksr_amd/mesh_simplify.py, csrc/meshsimp.hip) against the numpy fp64 restatement
(tests/mesh_simplify_ref.py).  Cluster ids, the vertex map, the faces and the four counts are compared exactly, index for index; the
representatives and colours within the bound derived next to REP_RTOL_OF_CELL.  Every test prints its maximum error before it asserts."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_geometry_ref as G
import mesh_simplify_ref as S
import mesh_topology_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Representatives, in units of the cell size.  The kernel and the restatement add the same terms in different orders.  A cluster's sums
# run over <= 3e4 terms (the longest row of these tests: the 27 648 corners of the torus in one cell) of magnitude <= tau * cell, and
# every step rounds by 2^-53: <= 3e4 * 1.1e-16 = 3.4e-12 of tau * cell in the right-hand side and of tau in the matrix.  The solve
# with (A + mu tau I) amplifies that by <= 1 / (2 sqrt(mu)) ~ 16 (mu = 1e-3) in the weakly constrained directions and by <= 1 in the
# others: 16 * 3.4e-12 * 2 (matrix and right-hand side) ~ 1.1e-10 of a cell.  1e-9 leaves a factor of 9.
REP_RTOL_OF_CELL = 1e-9
COLOUR_ATOL = 1e-12             # means of <= 5e3 values in [0, 1]: 5e3 * 2^-53 = 5.6e-13
FP32_ULP = 2.0 ** -23           # a result handed back as fp32 is rounded once more: one ulp at its magnitude on top of the bound
CUBE_SHIFT_ATOL = 1e-8          # p - centre rounds at 1e6 * 2^-53 = 1.1e-10 and is amplified by at most 16

CELLS = {'sphere': (0.02, 0.05, 0.1, 0.3), 'torus': (0.02, 0.05, 0.1, 0.3), 'shell': (0.02, 0.05, 0.1, 0.3, 2.0), 'holed': (0.02, 0.05, 0.1, 0.3),
         'soup': (0.02, 0.05, 0.1, 0.3), 'floaters': (0.02, 0.05, 0.1, 0.3)}
EXACT_CASES = [(name, cell) for name in CELLS for cell in CELLS[name]]
COUNTS = ('n_clusters', 'invalid_faces', 'collapsed_faces', 'duplicate_faces')


def _simplifier(v, f, colors=None):
    from nksr_amd.mesh_simplify import MeshSimplifier
    return MeshSimplifier(v, f, colors)


def _np(x):
    return x.cpu().numpy()


@functools.lru_cache(maxsize=None)
def mesh(name, vdt='float32'):
    """The shared meshes with colours (built once; nothing changes them).  The fp64 variant is not representable in fp32."""
    if name == 'sphere':
        v, f = T.uv_sphere(64, 32)
    elif name == 'torus':
        v, f = T.torus(96, 48)
    elif name == 'shell':
        v, f = T.voxel_mesh(T.voxel_sets()['shell'], 0)
    elif name == 'holed':
        v, f = G.holed_sphere()
    elif name == 'soup':                    # invalid faces, repeated faces, unreferenced vertices
        v, f = T.random_soup(3000, 200)
        v = np.concatenate([v[:100], np.random.RandomState(2).uniform(-3, 3, (5, 3)).astype(np.float32), v[100:]])      # five that no face names
        f = np.where(f >= 100, f + 5, f)
    elif name == 'floaters':
        v, f = T.sphere_with_floaters()[:2]
    elif name == 'strip254':                # V = 256: exactly one block of vertices
        v, f = T.triangle_strip(254)
    elif name == 'strip255':                # V = 257: one lane in the second block
        v, f = T.triangle_strip(255)
    else:
        raise KeyError(name)
    col = np.random.RandomState(11).uniform(0, 1, (len(v), 3))
    if vdt == 'float64':
        return v.astype(np.float64) * 1.0000001, f, col
    return v.astype(np.float32), f, col.astype(np.float32)


@functools.lru_cache(maxsize=None)
def ref(name, cell, vdt='float32', placement='quadric', dedup=True, origin=None):
    v, f, col = mesh(name, vdt)
    return S.simplify(v, f, cell, colors=col, placement=placement, dedup=dedup, origin=origin)


def _check_exact(r, want, fdt=None):
    assert np.array_equal(_np(r.cluster_id), want['cluster_id'])
    assert r.vertex_map.dtype == torch.int64 and np.array_equal(_np(r.vertex_map), want['vertex_map'])
    assert np.array_equal(_np(r.f2), want['f2']) and r.f2.shape == want['f2'].shape
    if fdt is not None:
        assert _np(r.f2).dtype == fdt
    got = {k: getattr(r, k) for k in COUNTS}
    assert got == {k: want[k] for k in COUNTS}, (got, {k: want[k] for k in COUNTS})
    assert r.cell_size == want['cell_size']


def _check_float(r, want, cell, label):
    """v2 / c2 against the restatement: the derived bound, plus one fp32 ulp where the result is handed back in fp32."""
    v2, c2 = _np(r.v2), _np(r.c2)
    assert v2.dtype == want['v2'].dtype and c2.dtype == want['c2'].dtype and v2.shape == want['v2'].shape and c2.shape == want['c2'].shape
    if v2.shape[0] == 0:
        print('%s: no vertices' % label)
        return
    fp32 = v2.dtype == np.float32
    ev = np.abs(v2.astype(np.float64) - want['v2_f64'])
    ec = np.abs(c2.astype(np.float64) - want['c2_f64'])
    bound_v = REP_RTOL_OF_CELL * cell + (FP32_ULP * np.abs(want['v2_f64']) if fp32 else 0.0)
    bound_c = COLOUR_ATOL + (FP32_ULP * np.abs(want['c2_f64']) if c2.dtype == np.float32 else 0.0)
    print('%s: max |v2 - ref| = %.3e (%.3e of a cell; bound %.3e of a cell%s), max |c2 - ref| = %.3e'
          % (label, ev.max(), ev.max() / cell, REP_RTOL_OF_CELL, ' + an fp32 ulp' if fp32 else '', ec.max()))
    assert (ev <= bound_v).all() and (ec <= bound_c).all()


# ---- against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, cell', EXACT_CASES)
def test_clusters_faces_and_counts_equal_the_restatement(name, cell):
    for vdt in ('float32', 'float64'):
        v, f, col = mesh(name, vdt)
        want = ref(name, cell, vdt)
        for fdt in (np.int32, np.int64):
            s = _simplifier(v, f.astype(fdt), col)
            r = s.simplify(cell_size=cell)
            _check_exact(r, want, fdt)
            _check_float(r, want, cell, '%s %g %s %s' % (name, cell, vdt, np.dtype(fdt).name))
            assert s.count_faces(cell) == r.f2.shape[0] == len(want['f2'])
    if name == 'soup':
        assert want['invalid_faces'] > 0 and (want['cluster_id'] < 0).any()
    if (name, cell) == ('torus', 0.3):
        assert want['duplicate_faces'] == 10 and len(want['f2']) == 10


@pytest.mark.parametrize('name, cell', [('sphere', 0.1), ('soup', 0.1), ('shell', 2.0)])
def test_mean_placement_no_dedup_and_torch_input(name, cell):
    v, f, col = mesh(name, 'float64')
    s = _simplifier(torch.from_numpy(v).cuda(), torch.from_numpy(f), torch.from_numpy(col))
    for placement, dedup in (('mean', True), ('quadric', False), ('mean', False)):
        want = ref(name, cell, 'float64', placement, dedup)
        r = s.simplify(cell_size=cell, placement=placement, dedup=dedup)
        _check_exact(r, want)
        _check_float(r, want, cell, '%s %s dedup=%s' % (name, placement, dedup))
        assert s.count_faces(cell, dedup=dedup) == len(want['f2'])
    assert s.simplify(cell_size=cell, dedup=False).duplicate_faces == 0


def test_regularisation_is_passed_on():
    v, f, col = mesh('holed', 'float64')
    s = _simplifier(v, f, col)
    for mu in (1.0, 1e-2):      # the bound's amplification 1 / (2 sqrt(mu)) only shrinks for mu > 1e-3
        want = S.simplify(v, f, 0.1, colors=col, regularisation=mu)
        _check_float(s.simplify(cell_size=0.1, regularisation=mu), want, 0.1, 'holed mu=%g' % mu)


def test_rotated_cube_at_an_offset_of_a_million():
    v, f = S.rotated_cube()
    far = S.rotated_cube(1e6)[0]
    want, want_far = S.simplify(v, f, 2.5), S.simplify(far, f, 2.5)
    r, r_far = _simplifier(v, f).simplify(cell_size=2.5), _simplifier(far, f).simplify(cell_size=2.5)
    _check_exact(r, want)
    _check_exact(r_far, want_far)
    assert r.n_clusters == 160 and r.f2.shape[0] == 318 and r.c2 is None
    e0 = np.abs(_np(r.v2) - want['v2_f64']).max()
    e1 = np.abs(_np(r_far.v2) - want_far['v2_f64']).max()
    e2 = np.abs(_np(r_far.v2) - 1e6 - _np(r.v2)).max()
    print('cube: max |v2 - ref| = %.3e; at 1e6: %.3e; shifted back against unshifted: %.3e; corner distance %.3e'
          % (e0, e1, e2, S.corner_error(_np(r_far.v2), 1e6)))
    assert e0 <= REP_RTOL_OF_CELL * 2.5 and e1 <= CUBE_SHIFT_ATOL and e2 <= CUBE_SHIFT_ATOL
    assert np.array_equal(_np(r.f2), _np(r_far.f2))
    mean = _simplifier(far, f).simplify(cell_size=2.5, placement='mean')
    assert 10 * S.corner_error(_np(r_far.v2), 1e6) <= S.corner_error(_np(mean.v2), 1e6)


# ---- edge shapes -------------------------------------------------------------------------------------------------------------------
def _empty_result(r, nv):
    assert r.v2.shape == (0, 3) and r.f2.shape == (0, 3) and r.vertex_map.shape == (nv,) and bool((r.vertex_map == -1).all())
    assert r.duplicate_faces == 0


def test_meshes_without_a_valid_face():
    r = _simplifier(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)).simplify(cell_size=1.0)
    _empty_result(r, 0)
    assert (r.n_clusters, r.invalid_faces, r.collapsed_faces) == (0, 0, 0)
    s = _simplifier(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((4, 2), np.float32))
    r = s.simplify(cell_size=1.0)
    _empty_result(r, 4)
    assert r.c2.shape == (0, 2) and r.f2.dtype == torch.int32 and s.count_faces(1.0) == 0
    assert s.simplify(target_faces=10).f2.shape[0] == 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)          # all faces invalid: NaN is unreferenced
    r = _simplifier(v, np.array([[0, 0, 1], [0, 1, 4], [-1, 1, 2], [2, 2, 2]])).simplify(cell_size=0.25)
    _empty_result(r, 4)
    assert (r.n_clusters, r.invalid_faces, r.collapsed_faces) == (0, 4, 0)


def test_one_triangle():
    v = np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 2, 0]], np.float32)
    f = np.array([[3, 0, 2]], np.int64)
    col = np.arange(8, dtype=np.float64).reshape(4, 2)
    want = S.simplify(v, f, 0.75, colors=col)
    r = _simplifier(v, f, col).simplify(cell_size=0.75)
    _check_exact(r, want)
    _check_float(r, want, 0.75, 'triangle')
    assert r.f2.shape[0] == 1 and _np(r.vertex_map).tolist()[1] == -1
    # a flat cluster: the quadric pins the normal direction, the regulariser pulls to the mean inside the plane: the vertices stay put
    assert np.abs(_np(r.v2)[_np(r.vertex_map)[[0, 2, 3]]] - v[[0, 2, 3]]).max() <= 1e-6
    _empty_result(_simplifier(v, f).simplify(cell_size=4.0), 4)                            # one cluster: the triangle collapses


@pytest.mark.parametrize('name', ['strip254', 'strip255'])
def test_one_block_of_vertices_and_one_lane_more(name):
    v, f, col = mesh(name)
    assert len(v) in (256, 257)
    for cell in (0.7, 3.0):
        want = S.simplify(v, f, cell, colors=col)
        r = _simplifier(v, f, col).simplify(cell_size=cell)
        _check_exact(r, want)
        _check_float(r, want, cell, '%s %g' % (name, cell))


def test_one_cluster_of_all_corners():
    v, f, col = mesh('torus', 'float64')
    assert 3 * len(f) == 27648
    want = ref('torus', 2.0, 'float64')
    r = _simplifier(v, f, col).simplify(cell_size=2.0)
    _check_exact(r, want)
    _empty_result(r, len(v))
    assert r.n_clusters == 1 and r.collapsed_faces == len(f)
    # the representative of that one cluster is dropped with it; the mean placement of the same run is looked at through dedup=False
    from nksr_amd import mesh_simplify as ms
    s = _simplifier(v, f, col)
    origin, c, m, keep, _ = s._faces(2.0, None, True)
    rep = _np(ms.place(s.x, s.f, ms.corner_incidence(m.cluster_faces, m.valid, c.n), c, origin, 2.0, 1e-3, ms.SIMP_QUADRIC))
    e = np.abs(rep - want['representatives']).max()
    print('one cluster of 27 648 corners: |rep - ref| = %.3e (%.3e of a cell)' % (e, e / 2.0))
    assert rep.shape == (1, 3) and e <= REP_RTOL_OF_CELL * 2.0
    ec = np.abs(_np(ms.cluster_means(s.colors, c)) - col.mean(0)).max()
    print('mean colour of 4 608 vertices: |c - ref| = %.3e' % ec)
    assert ec <= COLOUR_ATOL


def test_every_vertex_its_own_cluster():
    v, f, col = mesh('sphere')
    cell = 1e-4
    want = ref('sphere', cell)
    r = _simplifier(v, f, col).simplify(cell_size=cell)
    _check_exact(r, want)
    _check_float(r, want, cell, 'sphere 1e-4')
    assert r.n_clusters == len(v) and r.f2.shape[0] == len(f) and r.collapsed_faces == 0
    vmap = _np(r.vertex_map)                                                               # the compacted input, reordered by key
    assert np.array_equal(np.sort(vmap), np.arange(len(v))) and np.array_equal(_np(r.f2), vmap[f])
    # centre + (x - centre) rounds in fp64 (an exact 0 comes back as 7e-21), and the result is rounded to fp32 once more
    e = np.abs(_np(r.v2)[vmap].astype(np.float64) - v)
    print('sphere 1e-4: max |v2 - v| = %.3e' % e.max())
    assert (e <= 1e-12 * cell + FP32_ULP * np.abs(v)).all() and np.array_equal(_np(r.c2)[vmap], col)


def test_the_grid_limit_and_the_caller_origin():
    v = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [2097151.25, 0, 0], [2097151.5, 0.5, 0], [2097151.75, 0, 0.5]], np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    want = S.simplify(v, f, 1.0)
    s = _simplifier(v, f)
    r = s.simplify(cell_size=1.0)                                                          # the far triangle at index 2^21 - 1
    _check_exact(r, want)
    assert r.n_clusters == 2 and r.collapsed_faces == 2
    with pytest.raises(ValueError, match='extent'):                                        # ... at index 4 (2^21 - 1) + 1
        s.simplify(cell_size=0.25)
    far = v + np.array([[0, 0, 0]] * 3 + [[0.75, 0, 0]] * 3)                               # index exactly 2^21
    with pytest.raises(ValueError, match='2097153'):
        _simplifier(far, f).simplify(cell_size=1.0)
    with pytest.raises(ValueError, match='extent'):
        _simplifier(far, f).count_faces(1.0)
    sv, sf, col = mesh('sphere', 'float64')
    s = _simplifier(sv, sf, col)
    lo = sv.min(0)
    for bad in ([lo[0] + 1e-9, lo[1], lo[2]], [lo[0], lo[1], 0.0]):
        with pytest.raises(ValueError, match='origin'):
            s.simplify(cell_size=0.1, origin=bad)
    with pytest.raises(ValueError, match='origin'):
        s.simplify(cell_size=0.1, origin=[0.0, float('nan'), 0.0])
    below = (-0.43, -0.47, -0.41)
    want = ref('sphere', 0.1, 'float64', origin=below)
    r = s.simplify(cell_size=0.1, origin=below)
    _check_exact(r, want)
    _check_float(r, want, 0.1, 'sphere with a caller origin')
    assert s.count_faces(0.1, origin=np.array(below)) == len(want['f2']) != len(ref('sphere', 0.1, 'float64')['f2'])
    _check_exact(s.simplify(cell_size=0.1, origin=list(lo)), ref('sphere', 0.1, 'float64'))


def test_non_finite_coordinates_of_referenced_vertices():
    v, f, _ = mesh('sphere')
    bad = v.copy()
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        _simplifier(bad, f)


# ---- the target size ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target', [3000, 500, 50, 0])
def test_target_faces_replays_the_bisection(target):
    v, f, col = mesh('sphere')
    s = _simplifier(v, f, col)
    diag = S.diagonal(v, f)
    assert s.diagonal == diag
    h, steps = S.target_cell_size(lambda c: S.count_faces(v, f, c), diag, target)
    r = s.simplify(target_faces=target)
    print('target %d: cell_size %.17g (restatement %.17g), %d faces' % (target, r.cell_size, h, r.f2.shape[0]))
    assert steps == 24 and r.cell_size == h                                                # counts are exact: the floats agree bit for bit
    assert r.f2.shape[0] <= target and r.f2.shape[0] == S.count_faces(v, f, h)
    _check_exact(r, S.simplify(v, f, h, colors=col))


def test_a_target_above_the_face_count_returns_the_finest_grid():
    v, f, _ = mesh('sphere')
    r = _simplifier(v, f).simplify(target_faces=len(f))
    assert r.cell_size == S.diagonal(v, f) / 2.0 ** 20 and r.f2.shape[0] == len(f)


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, cell', [('floaters', 0.05), ('soup', 0.3), ('torus', 0.1)])
def test_two_runs_agree_bit_for_bit(name, cell):
    v, f, col = mesh(name, 'float64')
    a = _simplifier(v, f, col).simplify(cell_size=cell)
    b = _simplifier(v, f, col).simplify(cell_size=cell)
    assert torch.equal(a.v2, b.v2) and torch.equal(a.c2, b.c2) and torch.equal(a.f2, b.f2) and torch.equal(a.vertex_map, b.vertex_map)


@pytest.mark.parametrize('name, cell', [('floaters', 0.05), ('soup', 0.3)])
def test_a_shuffled_mesh_gives_the_same_clusters(name, cell):
    v, f, col = mesh(name, 'float64')
    seed = 3
    pv = np.random.RandomState(seed).permutation(len(v))                                   # the permutation T.shuffled draws first
    v2, f2 = T.shuffled(v, f, seed)
    assert np.array_equal(v2, v[pv])
    a = _simplifier(v, f, col).simplify(cell_size=cell)
    b = _simplifier(v2, f2, col[pv]).simplify(cell_size=cell)
    assert a.n_clusters == b.n_clusters and np.array_equal(_np(a.cluster_id)[pv], _np(b.cluster_id))
    assert (a.invalid_faces, a.collapsed_faces, a.duplicate_faces) == (b.invalid_faces, b.collapsed_faces, b.duplicate_faces)
    fa, fb = np.sort(_np(a.f2), axis=1), np.sort(_np(b.f2), axis=1)                        # (of equal triples another orientation may stay)
    assert np.array_equal(np.unique(fa, axis=0), np.unique(fb, axis=0)) and len(fa) == len(fb)
    ev, ec = np.abs(_np(a.v2) - _np(b.v2)).max(), np.abs(_np(a.c2) - _np(b.c2)).max()
    print('%s shuffled: max |v2 - v2\'| = %.3e (%.3e of a cell), colours %.3e' % (name, ev, ev / cell, ec))
    assert ev <= REP_RTOL_OF_CELL * cell and ec <= COLOUR_ATOL


# ---- invariants without the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', [0.05, 0.1, 0.2])
def test_the_simplified_sphere_is_watertight_and_every_vertex_stays_in_its_cell(cell):
    from nksr_amd.mesh_topology import MeshTopology
    v, f, _ = mesh('sphere', 'float64')
    r = _simplifier(v, f).simplify(cell_size=cell)
    t = MeshTopology(r.v2, r.f2)
    assert t.is_watertight and t.euler_characteristic == 2 and t.invalid_faces == 0 and t.referenced_vertices == r.v2.shape[0]
    assert 0 < r.f2.shape[0] < len(f)
    vmap, out = _np(r.vertex_map), _np(r.v2)
    assert (vmap >= 0).all()
    lo = v.min(0)
    cells = np.floor((v - lo) / cell)
    centre = lo + (cells + 0.5) * cell
    excess = np.abs(out[vmap] - centre).max() - 0.5 * cell
    slack = 4 * 2.0 ** -53 * np.abs(v).max()                # centre + x and the centre itself round at the coordinates' magnitude
    print('cell %g: max |v2 - centre| - cell / 2 = %.3e (slack %.3e)' % (cell, excess, slack))
    assert excess <= slack


@pytest.mark.parametrize('name, cell', [('torus', 0.3), ('soup', 0.3), ('soup', 0.05), ('sphere', 0.1)])
def test_duplicates_account_for_the_difference_of_the_two_counts(name, cell):
    v, f, _ = mesh(name)
    s = _simplifier(v, f)
    r = s.simplify(cell_size=cell)
    print('%s %g: %d faces without dedup, %d duplicates' % (name, cell, s.count_faces(cell, dedup=False), r.duplicate_faces))
    assert s.count_faces(cell, dedup=False) - r.duplicate_faces == s.count_faces(cell) == r.f2.shape[0]
    if name != 'sphere':
        assert r.duplicate_faces > 0


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_meshing_result_simplify_end_to_end():
    import nksr
    from conftest import make_cloud
    from nksr.metrics import MeshEvaluator
    from nksr_amd.fields.base_field import MeshingResult
    dev = torch.device('cuda:0')
    xyz, nrm = make_cloud('sphere', 3000, 0.005, 0)
    rec = nksr.Reconstructor(dev, config='snet-n3k-wnormal')
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=None)
    mesh0 = fld.extract_dual_mesh(mise_iter=1)
    voxel = rec.hparams.voxel_size / fld.scale
    coloured = MeshingResult(mesh0.v, mesh0.f, (mesh0.v * 0.5 + 0.5).clamp(0, 1))
    small = coloured.simplify(cell_size=3 * voxel)
    print('recipe mesh: V %d F %d -> V %d F %d at %g' % (mesh0.v.shape[0], mesh0.f.shape[0], small.v.shape[0], small.f.shape[0], 3 * voxel))
    assert isinstance(small, MeshingResult) and 0 < small.f.shape[0] < mesh0.f.shape[0] and small.v.shape[0] < mesh0.v.shape[0]
    assert small.v.dtype == mesh0.v.dtype and small.f.dtype == mesh0.f.dtype and small.c.shape == (small.v.shape[0], 3)
    # a cell's mean colour is the colour of the cell's mean vertex, which lies within one cell of the representative (and fp32 rounding)
    assert float((small.c - (small.v * 0.5 + 0.5)).abs().max()) <= 0.5 * 3 * voxel + 1e-6
    assert mesh0.simplify(cell_size=3 * voxel).c is None
    by_target = mesh0.simplify(target_faces=small.f.shape[0])
    assert 0 < by_target.f.shape[0] <= small.f.shape[0]
    gt, gtn = make_cloud('sphere', 50000, 0.0, 12345)
    m = MeshEvaluator(50000, ['chamfer-L1', 'f-score']).eval_mesh(small, gt, gtn)
    print('simplified recipe mesh:', m)
    assert math.isfinite(m['chamfer-L1']) and 0.0 <= m['f-score'] <= 1.0


def test_recons_simplified_example(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'recons_simplified.py')], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    sizes = [[int(t.split('=')[1]) for t in line.split()[:2]] for line in out.stdout.splitlines() if line.startswith('V=')]
    print(out.stdout)
    assert len(sizes) == 2 and 0 < sizes[1][1] < sizes[0][1] and (tmp_path / 'recons_simplified.ply').exists()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    v, f, col = mesh('sphere')
    s = _simplifier(v, f, col)
    for bad in (0.0, -0.1, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='cell_size'):
            s.simplify(cell_size=bad)
        with pytest.raises(ValueError, match='cell_size'):
            s.count_faces(bad)
    with pytest.raises(ValueError, match='target_faces'):
        s.simplify(target_faces=-1)
    for mu in (0.0, -1e-3, 1.5, float('nan')):
        with pytest.raises(ValueError, match='regularisation'):
            s.simplify(cell_size=0.1, regularisation=mu)
    with pytest.raises(ValueError, match='placement'):
        s.simplify(cell_size=0.1, placement='median')
    with pytest.raises(ValueError, match='exactly one'):
        s.simplify()
    with pytest.raises(ValueError, match='exactly one'):
        s.simplify(cell_size=0.1, target_faces=100)
    for bad in ((col * 255).astype(np.uint8), col > 0.5, (col * 255).astype(np.int64)):
        with pytest.raises(ValueError, match='colors'):
            _simplifier(v, f, bad)
    with pytest.raises(ValueError, match='colors'):
        _simplifier(v, f, col[:-1])
    with pytest.raises(ValueError, match='faces'):
        _simplifier(v, f.astype(np.float32))
    with pytest.raises(ValueError):
        _simplifier(v[:, :2], f)
    with pytest.raises(RuntimeError):
        _simplifier(v, f).__class__(v, f, device='cpu')
