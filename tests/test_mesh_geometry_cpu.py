"""The numpy / scipy restatement of the mesh geometry (tests/mesh_geometry_ref.py) against closed-form answers -- it has to earn its
place as the yardstick of tests/test_gpu_mesh_geometry.py -- and the argument errors of the C ABI of csrc/meshgeom.hip and the
exports, without a GPU."""
import numpy as np

import mesh_geometry_ref as G
import mesh_topology_ref as T

SPHERE_R = 0.4


def test_angle_defects_of_the_tetrahedron_and_the_cube():
    v, f = T.tetrahedron((0.1, -0.2, 0.3), 0.5)
    assert np.allclose(G.gaussian_curvature(v, f, integrated=True), np.pi, rtol=0, atol=1e-6)          # (fp32 vertices)
    v, f = T.tetrahedron((0, 0, 0), 1.0)                                                                # exact in fp32
    assert np.abs(G.gaussian_curvature(v, f, integrated=True) - np.pi).max() < 1e-14
    for seed in range(4):                                               # every corner pi / 2 however the squares were split
        v, f = T.voxel_mesh({(0, 0, 0)}, seed)
        k = G.gaussian_curvature(v, f, integrated=True)
        assert len(v) == 8 and np.abs(k - np.pi / 2).max() < 1e-14, seed


def test_gauss_bonnet_areas_and_the_closed_surface_identity():
    cases = ((T.uv_sphere(64, 32), 2), (T.torus(96, 48), 0), (T.voxel_mesh(T.voxel_sets()['shell'], 0), 4))
    for (v, f), chi in cases:
        assert T.edge_table(f, len(v))['euler'] == chi
        total = G.gaussian_curvature(v, f, integrated=True).sum()
        print('chi', chi, 'Gauss-Bonnet residual', abs(total - 2 * np.pi * chi))
        assert abs(total - 2 * np.pi * chi) < 1e-9
        face_area = G.face_quantities(v, f)[4].sum()
        assert abs(G.vertex_areas(v, f).sum() - face_area) <= 1e-12 * face_area
        terms = G.weighted_laplacian(v, f)                              # 2 A_i Delta x_i: sums to zero over a closed surface
        assert np.abs(terms.sum(0)).max() <= 1e-12 * np.abs(terms).max()
    v, f = T.voxel_mesh(T.voxel_sets()['shell'], 0)
    assert abs(G.gaussian_curvature(v, f, integrated=True).sum() - 8 * np.pi) < 1e-9


def test_sphere_curvatures_and_normals():
    v, f = T.uv_sphere(64, 32)
    band = np.abs(v[:, 2]) < 0.8 * SPHERE_R
    h, k = G.mean_curvature(v, f) * SPHERE_R, G.gaussian_curvature(v, f) * SPHERE_R ** 2
    print('H r', h[band].min(), h[band].max(), 'K r^2', k[band].min(), k[band].max())
    assert not np.isnan(h).any() and not np.isnan(k).any()
    assert 0.99 <= h[band].min() and h[band].max() <= 1.01
    assert 0.99 <= k[band].min() and k[band].max() <= 1.01
    for weighting in ('angle', 'area'):
        n = G.vertex_normals(v, f, weighting)
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-14
        assert ((n * v).sum(1) > 0.99 * SPHERE_R).all(), weighting
    # inward orientation flips the normals and the sign of H
    assert (G.mean_curvature(v, f[:, ::-1])[band] < 0).all()


def test_borders_unreferenced_vertices_and_invalid_faces():
    v, f = G.holed_sphere()
    a = G.adjacency(f, len(v))
    on_border = a['vertex_kind'] == G.ON_BOUNDARY
    assert 0 < on_border.sum() < 40 and (a['vertex_kind'] != G.UNREFERENCED).all()
    for x in (G.gaussian_curvature(v, f), G.mean_curvature(v, f)):
        assert np.array_equal(np.isnan(x), on_border)
    v2 = np.concatenate([v, [[9, 9, 9]]]).astype(np.float32)
    f2 = np.concatenate([f, [[0, 0, 5], [1, 2, len(v2)]]])
    b = G.adjacency(f2, len(v2))
    assert b['vertex_kind'][-1] == G.UNREFERENCED and np.array_equal(b['neighbours'], a['neighbours'])
    assert np.array_equal(G.vertex_normals(v2, f2)[:-1], G.vertex_normals(v, f)) and (G.vertex_normals(v2, f2)[-1] == 0).all()
    assert np.isnan(G.mean_curvature(v2, f2)[-1]) and G.vertex_areas(v2, f2)[-1] == 0
    # rows ascend, the degree is the row length, the three_fan's edge (0, 1) appears once per direction
    v, f = T.three_fan()
    c = G.adjacency(f, len(v))
    assert c['neighbours'].tolist() == [1, 2, 3, 4, 0, 2, 3, 4, 0, 1, 0, 1, 0, 1] and c['vertex_degree'].tolist() == [4, 4, 2, 2, 2]
    assert c['neighbour_start'].tolist() == [0, 4, 8, 10, 12, 14] and (c['vertex_kind'] == G.ON_BOUNDARY).all()


def test_laplacian_shrinks_and_taubin_does_not():
    v, f = T.uv_sphere(64, 32)
    x = G.noisy(v, 0.004)
    r0 = np.linalg.norm(x.astype(np.float64), axis=1).mean()
    lap = np.linalg.norm(G.smooth(x, f, 10, 'laplacian'), axis=1).mean()
    tau = np.linalg.norm(G.smooth(x, f, 5, 'taubin'), axis=1).mean()
    print('mean radius: noisy', r0, 'laplacian x10', lap, 'taubin x5', tau)
    assert r0 - lap > r0 - tau and r0 - lap > 0
    assert np.array_equal(G.smooth(x, f, 0), x.astype(np.float64))
    # pinned vertices and the three boundary modes on the holed sphere
    v, f = G.holed_sphere()
    x = G.noisy(v, 0.004)
    border = G.adjacency(f, len(v))['vertex_kind'] == G.ON_BOUNDARY
    out = {b: G.smooth(x, f, 3, boundary=b) for b in ('fixed', 'curve', 'free')}
    assert np.array_equal(out['fixed'][border], x[border].astype(np.float64))
    assert (out['curve'][border] != x[border]).any(1).all() and (out['free'][border] != out['curve'][border]).any()
    mask = np.arange(len(v)) % 7 == 0
    assert np.array_equal(G.smooth(x, f, 3, fixed=mask)[mask], x[mask].astype(np.float64))


def test_geometry_c_abi_argument_errors_without_a_gpu():
    """Argument validation happens before any launch: error code + message on a machine without a GPU, never an abort."""
    import ctypes as C
    from nksr_amd import _lib
    lib, null = _lib.lib, C.c_void_p(0)

    def err():
        return lib.nksr_last_error().decode()

    i64, dbl = C.c_int64, C.c_double
    one = (C.c_int64 * 16)()
    two = (C.c_int64 * 16)()
    big, E = i64((1 << 30) + 1), _lib.ERR_ARG
    assert lib.nksr_geom_directed_keys(null, i64(5), i64(9), null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_directed_keys(one, i64(-5), i64(9), one, one, null) == E and 'negative' in err()
    assert lib.nksr_geom_directed_keys(one, i64(5), i64(1 << 31), one, one, null) == E and '2^31' in err()
    assert lib.nksr_geom_directed_keys(one, i64(1 << 31), i64(9), one, one, null) == E and '2^31' in err()
    assert lib.nksr_geom_directed_keys(null, i64(0), i64(9), null, null, null) == 0
    assert lib.nksr_geom_adjacency(null, null, i64(5), i64(9), null, null, null, null, null, null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_adjacency(one, one, i64(5), i64(-9), one, one, one, one, one, one, one, null) == E and 'negative' in err()
    assert lib.nksr_geom_corner_keys(null, 0, i64(5), i64(9), null, null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_corner_keys(one, 0, big, i64(9), one, one, one, null) == E and '2^30' in err()
    assert lib.nksr_geom_corner_keys(null, 0, i64(0), i64(9), null, null, null, null) == 0
    assert lib.nksr_geom_corner_rows(one, i64(7), i64(9), one, null) == E and 'three times' in err()
    assert lib.nksr_geom_corner_rows(null, i64(6), i64(9), null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_corner_rows(one, i64(3 * ((1 << 30) + 1)), i64(9), one, null) == E and '2^30' in err()
    assert lib.nksr_geom_faces(null, 0, i64(9), null, 0, i64(5), null, null, null, null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_faces(one, 0, i64(1 << 31), one, 0, i64(5), one, one, one, one, one, null) == E and '2^31' in err()
    assert lib.nksr_geom_faces(null, 0, i64(9), null, 0, i64(0), null, null, null, null, null, null) == 0
    assert lib.nksr_geom_edge_weights(null, null, i64(3), i64(2), null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_edge_weights(one, one, i64(7), i64(2), one, one, null) == E and 'n_edges' in err()
    assert lib.nksr_geom_edge_weights(one, one, i64(3), big, one, one, null) == E and '2^30' in err()
    assert lib.nksr_geom_vertex_gather(null, null, i64(9), i64(5), null, null, null, 0, null, null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_vertex_gather(one, one, i64(9), i64(5), one, one, one, 0, null, null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_vertex_gather(one, one, i64(9), i64(5), one, one, one, 2, one, one, one, null) == E and 'weighting' in err()
    assert lib.nksr_geom_vertex_gather(null, null, i64(0), i64(0), null, null, null, 1, null, null, null, null) == 0
    assert lib.nksr_geom_curvature(null, 0, i64(9), null, null, null, i64(5), null, null, null, null, null, null, null) == E and 'NULL' in err()
    assert lib.nksr_geom_curvature(one, 0, i64(9), one, one, one, i64(5), one, one, null, one, null, one, null) == E and 'NULL' in err()
    assert lib.nksr_geom_curvature(one, 0, i64(9), one, one, one, i64(-5), one, one, one, one, one, one, null) == E and 'negative' in err()
    args = [one, two, i64(9), one, one, i64(5), one, one, null, 0, i64(4), dbl(0.5), dbl(-0.53), null]
    for k in (0, 1, 3, 4, 6, 7):
        bad = list(args)
        bad[k] = null
        assert lib.nksr_geom_smooth(*bad) == E and 'NULL' in err(), k
    for k, value, word in ((9, 3, 'boundary'), (10, i64(-1), 'negative'), (2, i64(1 << 31), '2^31'), (1, one, 'same buffer')):
        bad = list(args)
        bad[k] = value
        assert lib.nksr_geom_smooth(*bad) == E and word in err(), (k, err())
    args[10] = i64(0)                                                   # no steps, or no vertices: nothing is launched
    assert lib.nksr_geom_smooth(*args) == 0
    assert lib.nksr_geom_smooth(null, null, i64(0), null, null, i64(0), null, null, null, 2, i64(4), dbl(0.5), dbl(0.5), null) == 0


def test_exports_and_host_side_argument_checks():
    import nksr
    from nksr_amd import build
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_geometry import MeshGeometry
    assert 'MeshGeometry' in nksr.__all__ and nksr.MeshGeometry is MeshGeometry and nksr.metrics.MeshGeometry is MeshGeometry
    assert 'meshgeom.hip' in build.SOURCES
    for name in ('vertex_normals', 'smooth', 'geometry'):
        assert callable(getattr(MeshingResult, name))
    assert 'bit for bit' in __import__('nksr_amd.mesh_geometry').mesh_geometry.__doc__
