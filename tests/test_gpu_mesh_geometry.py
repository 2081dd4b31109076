"""Mesh geometry on the MI355X (nksr_amd/mesh_geometry.py, csrc/meshgeom.hip) against the numpy / scipy fp64 restatement
(tests/mesh_geometry_ref.py).  Adjacency, degree and vertex kind are compared exactly; the floating-point results within the bounds
written next to each constant below.  Every test prints its maximum error before it asserts."""
import functools

import numpy as np
import pytest
import torch

import mesh_geometry_ref as G
import mesh_topology_ref as T

pytestmark = pytest.mark.gpu

NORMAL_ATOL_F64 = 1e-12         # unit components from fp64 sums of <= 64 terms
NORMAL_ATOL_F32 = 2.0 ** -23    # one rounding of a unit component to fp32 (half an ulp at 1 = 2^-24) plus the fp64 noise
AREA_RTOL = 1e-12
GAUSS_RTOL, GAUSS_ATOL = 1e-12, 1e-11
MEAN_RTOL_OF_MAX = 1e-11        # of max |H|: the meshes' smallest angle is 5.6 degrees, which bounds the cotangents' conditioning
GAUSS_BONNET_ATOL = 1e-9
SMOOTH_RTOL_OF_DIAGONAL = 1e-11  # reorder error per step <= deg 2^-53 2 max|x|, times at most (1 + 2 |mu|) per pair: ~1e-12 for 5 pairs
SHIFT_ATOL = 1e-8               # fp64 state at coordinates of 1e6: 1e6 2^-53 per operation


def _geom(v, f):
    from nksr_amd.mesh_geometry import MeshGeometry
    return MeshGeometry(v, f)


def _np(x):
    return x.cpu().numpy()


def _u32(x):
    return _np(x).astype(np.int64) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The shared meshes (built once; nothing changes them)."""
    if name == 'sphere':
        return T.uv_sphere(64, 32)
    if name == 'torus':
        return T.torus(96, 48)
    if name == 'shell':
        return T.voxel_mesh(T.voxel_sets()['shell'], 0)
    if name == 'holed':
        return G.holed_sphere()
    if name == 'noisy_sphere':          # the pole has degree 64: long rows
        v, f = T.uv_sphere(64, 32)
        return G.noisy(v, 0.004), f
    if name == 'noisy_torus':
        v, f = T.torus(96, 48)
        return G.noisy(v, 0.004, seed=1), f
    if name == 'noisy_holed':
        v, f = G.holed_sphere()
        return G.noisy(v, 0.004, seed=2), f
    if name == 'fan':
        return T.three_fan()
    if name == 'cubes':
        return T.two_cubes_sharing_a_vertex()
    if name == 'soup':                  # invalid faces, repeated faces, non-manifold junk
        return T.random_soup(3000, 200)
    if name == 'strip254':              # V = 256: exactly one block of vertices
        return T.triangle_strip(254)
    if name == 'strip255':              # V = 257: one lane in the second block
        return T.triangle_strip(255)
    if name == 'empty0':
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    if name == 'empty4':
        return np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)
    if name == 'triangle':
        return np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 2, 0]], np.float32), np.array([[3, 0, 2]], np.int64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref_adjacency(name):
    v, f = mesh(name)
    return G.adjacency(f, len(v))


def _diagonal(v):
    return float(np.linalg.norm(np.ptp(np.asarray(v, np.float64), axis=0)))


# ---- adjacency -------------------------------------------------------------------------------------------------------------------
def _check_adjacency(g, ref):
    assert np.array_equal(_u32(g.neighbour_start), ref['neighbour_start'])
    assert g.neighbours.dtype == torch.int32 and np.array_equal(_np(g.neighbours), ref['neighbours'])
    assert np.array_equal(_np(g.neighbour_edge), ref['neighbour_edge']) and np.array_equal(_np(g.neighbour_class), ref['neighbour_class'])
    assert np.array_equal(_np(g.vertex_degree), ref['vertex_degree'])
    assert g.vertex_kind.dtype == torch.uint8 and np.array_equal(_np(g.vertex_kind), ref['vertex_kind'])


@pytest.mark.parametrize('name', ['sphere', 'torus', 'shell', 'holed', 'fan', 'cubes', 'soup', 'strip254', 'strip255', 'empty0', 'empty4',
                                  'triangle'])
def test_adjacency_degree_and_kind_equal_the_restatement(name):
    v, f = mesh(name)
    g = _geom(v, f)
    ref = ref_adjacency(name)
    _check_adjacency(g, ref)
    assert g.neighbours.shape[0] == 2 * g.topology.num_edges and g.neighbour_start.shape[0] == len(v) + 1
    if name == 'holed':
        assert 0 < (ref['vertex_kind'] == G.ON_BOUNDARY).sum() < 40
    if name == 'triangle':
        assert _np(g.vertex_kind).tolist() == [1, 2, 1, 1] and _np(g.vertex_degree).tolist() == [2, 0, 2, 2]
    if name == 'soup':
        assert g.topology.invalid_faces > 0 and g.topology.nonmanifold_edges > 0
    if name in ('empty0', 'empty4'):
        assert g.neighbours.shape[0] == 0 and (_np(g.vertex_kind) == G.UNREFERENCED).all()
        assert g.vertex_normals().shape == (len(v), 3) and g.mean_curvature().shape == (len(v),) and g.smooth(3).shape == (len(v), 3)


def test_face_dtypes_and_from_topology():
    from nksr_amd.mesh_geometry import MeshGeometry
    from nksr_amd.mesh_topology import MeshTopology
    v, f = mesh('soup')
    ref = ref_adjacency('soup')
    a, b = _geom(v, f), _geom(torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int32)))
    assert a.f.dtype == torch.int64 and b.f.dtype == torch.int32
    _check_adjacency(b, ref)
    t = MeshTopology(v, f)
    c = MeshGeometry.from_topology(t)
    assert c.topology is t
    _check_adjacency(c, ref)
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x.vertex_normals(), y.vertex_normals()) and torch.equal(x.vertex_areas(), y.vertex_areas())


# ---- normals, areas, curvature -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['noisy_sphere', 'torus', 'noisy_holed', 'shell', 'cubes', 'soup'])
def test_vertex_normals_both_weightings_and_precisions(name):
    v, f = mesh(name)
    if name == 'noisy_holed':           # an unreferenced vertex and two invalid faces on top
        v = np.concatenate([v, [[9, 9, 9]]]).astype(np.float32)
        f = np.concatenate([f, [[0, 0, 5], [1, 2, len(v)]]])
    g32, g64 = _geom(v, f), _geom(v.astype(np.float64), f)
    for weighting in ('angle', 'area'):
        ref = G.vertex_normals(v, f, weighting)
        zero = (ref == 0).all(1)
        n64, n32 = g64.vertex_normals(weighting), g32.vertex_normals(weighting)
        assert n64.dtype == torch.float64 and n32.dtype == torch.float32 and n64.shape == n32.shape == (len(v), 3)
        e64, e32 = np.abs(_np(n64) - ref).max(), np.abs(_np(n32).astype(np.float64) - ref).max()
        print(name, weighting, 'max normal error: fp64 input %.3g, fp32 input %.3g; zero rows %d' % (e64, e32, zero.sum()))
        assert e64 <= NORMAL_ATOL_F64 and e32 <= NORMAL_ATOL_F32
        assert np.array_equal((_np(n64) == 0).all(1), zero) and np.array_equal((_np(n32) == 0).all(1), zero)
        assert np.abs(np.linalg.norm(_np(n64)[~zero], axis=1) - 1).max(initial=0) < 1e-14
    if name == 'noisy_holed':
        assert zero[-1] and zero.sum() == 1
    with pytest.raises(ValueError):
        g32.vertex_normals('uniform')


@pytest.mark.parametrize('name', ['sphere', 'noisy_sphere', 'torus', 'noisy_torus', 'holed', 'shell', 'cubes'])
def test_areas_and_curvatures(name):
    v, f = mesh(name)
    if name.startswith('noisy'):        # noise below 5 % of the shortest edge: the cotangents stay as well conditioned as the clean mesh's
        clean = mesh(name[len('noisy_'):])[0].astype(np.float64)
        e = T.edge_table(f, len(v))['edges']
        shortest = np.linalg.norm(clean[e[:, 0]] - clean[e[:, 1]], axis=1).min()
        v = (clean + np.random.RandomState(3).uniform(-1, 1, clean.shape) * 0.05 * shortest / np.sqrt(3)).astype(np.float32)
    g = _geom(v, f)
    area, ref_area = _np(g.vertex_areas()), G.vertex_areas(v, f)
    err = np.abs(area - ref_area) / np.maximum(ref_area, 1e-300)
    print(name, 'max relative vertex-area error %.3g' % err.max())
    assert area.dtype == np.float64 and (np.abs(area - ref_area) <= AREA_RTOL * ref_area).all()
    for integrated in (True, False):
        k, ref = _np(g.gaussian_curvature(integrated)), G.gaussian_curvature(v, f, integrated)
        assert np.array_equal(np.isnan(k), np.isnan(ref))
        ok = ~np.isnan(ref)
        print(name, 'integrated' if integrated else 'pointwise', 'max Gaussian curvature error %.3g (max |K| %.3g)' %
              (np.abs(k - ref)[ok].max(), np.abs(ref[ok]).max()))
        assert (np.abs(k - ref)[ok] <= GAUSS_ATOL + GAUSS_RTOL * np.abs(ref[ok])).all()
    h, ref = _np(g.mean_curvature()), G.mean_curvature(v, f)
    assert np.array_equal(np.isnan(h), np.isnan(ref))
    ok = ~np.isnan(ref)
    scale = np.abs(ref[ok]).max()
    print(name, 'max mean-curvature error %.3g of max |H| = %.3g; NaN at %d vertices' % (np.abs(h - ref)[ok].max() / scale, scale, (~ok).sum()))
    assert (np.abs(h - ref)[ok] <= MEAN_RTOL_OF_MAX * scale).all()
    if name == 'holed':
        assert np.array_equal(~ok, ref_adjacency('holed')['vertex_kind'] == G.ON_BOUNDARY)
    if name == 'sphere':                # positive on an outward-oriented sphere
        band = np.abs(v[:, 2]) < 0.8 * 0.4
        assert (h[band] * 0.4 > 0.99).all() and (h[band] * 0.4 < 1.01).all()
    lap = _np(g.cotangent_laplacian())
    with np.errstate(divide='ignore', invalid='ignore'):
        ref_lap = G.weighted_laplacian(v, f) / (2.0 * ref_area[:, None])
    assert (np.abs(lap - ref_lap)[ok] <= 2 * MEAN_RTOL_OF_MAX * scale).all() and np.isnan(lap[~ok]).all()


@pytest.mark.parametrize('name', ['sphere', 'torus', 'shell'])
def test_gauss_bonnet_on_the_gpu(name):
    g = _geom(*mesh(name))
    total = float(_np(g.gaussian_curvature(integrated=True)).sum())
    chi = g.topology.euler_characteristic
    print(name, 'chi', chi, 'Gauss-Bonnet residual %.3g' % abs(total - 2 * np.pi * chi))
    assert chi == {'sphere': 2, 'torus': 0, 'shell': 4}[name] and abs(total - 2 * np.pi * chi) <= GAUSS_BONNET_ATOL


# ---- smoothing ---------------------------------------------------------------------------------------------------------------------
SMOOTH_CASES = [('noisy_sphere', 'laplacian', 10, 'fixed', False), ('noisy_sphere', 'taubin', 5, 'fixed', False),
                ('noisy_torus', 'laplacian', 10, 'free', False), ('noisy_torus', 'taubin', 5, 'fixed', True),
                ('noisy_holed', 'taubin', 5, 'fixed', False), ('noisy_holed', 'taubin', 5, 'curve', False),
                ('noisy_holed', 'taubin', 5, 'free', False), ('noisy_holed', 'laplacian', 10, 'curve', True)]


@pytest.mark.parametrize('name,method,iterations,boundary,masked', SMOOTH_CASES)
def test_smoothing_equals_the_restatement(name, method, iterations, boundary, masked):
    v, f = mesh(name)
    fixed = (np.arange(len(v)) % 7 == 0) if masked else None
    kind = ref_adjacency(name)['vertex_kind']
    pinned = np.zeros(len(v), bool) if fixed is None else fixed.copy()
    if boundary == 'fixed':
        pinned |= kind == G.ON_BOUNDARY
    ref = G.smooth(v, f, iterations, method, boundary=boundary, fixed=fixed)
    diag = _diagonal(v)
    # fp64 input: the kernels' fp64 state against the restatement's
    v64 = v.astype(np.float64)
    out = _geom(v64, f).smooth(iterations, method, boundary=boundary, fixed=fixed)
    assert out.dtype == torch.float64 and out.shape == (len(v), 3)
    err = np.abs(_np(out) - ref).max()
    moved = np.abs(_np(out) - v64).max()
    print(name, method, boundary, 'masked' if masked else '', 'max error %.3g = %.3g of the diagonal; largest move %.3g' % (err, err / diag, moved))
    assert err <= SMOOTH_RTOL_OF_DIAGONAL * diag and moved > 1e-4
    assert np.array_equal(_np(out)[pinned].view(np.uint64), v64[pinned].view(np.uint64))
    assert (np.abs(_np(out) - v64)[~pinned & (kind != G.UNREFERENCED)].max(1) > 0).all()
    # fp32 input: one rounding at the end
    out32 = _geom(v, f).smooth(iterations, method, boundary=boundary, fixed=torch.from_numpy(fixed) if masked else None)
    ulp = float(np.spacing(np.float32(np.abs(v).max())))
    err32 = np.abs(_np(out32).astype(np.float64) - ref).max()
    print('    fp32 input: max error %.3g, one ulp of max|x| = %.3g' % (err32, ulp))
    assert out32.dtype == torch.float32 and err32 <= ulp
    assert np.array_equal(_np(out32)[pinned].view(np.uint32), v[pinned].view(np.uint32))


def test_smoothing_shrinkage_zero_iterations_and_the_shifted_sphere():
    v, f = mesh('noisy_sphere')
    g = _geom(v, f)
    r = lambda x: float(np.linalg.norm(_np(x).astype(np.float64), axis=1).mean())       # noqa: E731
    r0, lap, tau = r(g.v), r(g.smooth(10, 'laplacian')), r(g.smooth(5))
    print('mean radius: noisy %.6f, laplacian x10 %.6f, taubin x5 %.6f' % (r0, lap, tau))
    assert r0 - lap > abs(r0 - tau) and r0 - lap > 0.005
    for x in (v, v.astype(np.float64)):
        out = _geom(x, f).smooth(0)
        assert out.dtype == torch.from_numpy(x).dtype and np.array_equal(_np(out).view(np.uint8), x.view(np.uint8))
        assert out.data_ptr() != _geom(x, f).v.data_ptr()
    # fp64 vertices + 1e6: smoothed and shifted back they agree with the unshifted run (the state is fp64, nothing is recentred)
    v64 = v.astype(np.float64)
    plain = _np(_geom(v64, f).smooth(5))
    far = _np(_geom(v64 + 1e6, f).smooth(5)) - 1e6
    print('shifted by 1e6: max difference %.3g' % np.abs(far - plain).max())
    assert np.abs(far - plain).max() <= SHIFT_ATOL
    assert np.abs(plain - v64).max() > 1e-4


def test_two_builds_and_two_runs_are_bitwise_equal():
    v, f = mesh('noisy_holed')
    a, b = _geom(v, f), _geom(v, f)
    for k in ('neighbour_start', 'neighbours', 'neighbour_edge', 'neighbour_class', 'vertex_kind'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    bits = lambda x: x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)      # noqa: E731  (NaN compares equal)
    for fn in (lambda g: g.vertex_normals('angle'), lambda g: g.vertex_normals('area'), lambda g: g.vertex_areas(),
               lambda g: g.gaussian_curvature(), lambda g: g.mean_curvature(), lambda g: g.smooth(5, boundary='curve'),
               lambda g: g.smooth(4, 'laplacian', boundary='free')):
        x, y, z = fn(a), fn(b), fn(a)
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))


def test_errors_are_exceptions():
    v, f = mesh('fan')
    g = _geom(v, f)
    for kw in ({'method': 'cotangent'}, {'boundary': 'open'}, {'lam': 0.0}, {'lam': 1.5}, {'lam': -0.5}, {'mu': -0.5}, {'mu': 0.2},
               {'fixed': np.ones(3, bool)}, {'fixed': np.ones((len(v), 1), bool)}):
        with pytest.raises(ValueError):
            g.smooth(2, **kw)
    with pytest.raises(ValueError):
        g.smooth(-1)
    with pytest.raises(ValueError):
        g.vertex_normals('face')
    assert g.smooth(2, 'laplacian', lam=1.0, mu=5.0).shape == (len(v), 3)           # mu is Taubin's: not looked at here
    with pytest.raises(ValueError):
        _geom(v, f.astype(np.float32))
    with pytest.raises(ValueError):
        _geom(v, f.astype(bool))
    with pytest.raises(ValueError):
        _geom(v[:, :2], f)
    from nksr_amd.mesh_geometry import MeshGeometry
    with pytest.raises(RuntimeError):
        MeshGeometry(v, f, device='cpu')
    with pytest.raises(TypeError):
        MeshGeometry.from_topology((v, f))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_recipe_mesh_smoothing_and_normals():
    import nksr
    from conftest import make_cloud
    from nksr_amd.fields.base_field import MeshingResult
    dev = torch.device('cuda:0')
    xyz, nrm = make_cloud('sphere', 3000, 0.005, 0)
    rec = nksr.Reconstructor(dev, config='snet-n3k-wnormal')
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=None)
    mesh0 = fld.extract_dual_mesh(mise_iter=1)
    mesh0.c = torch.rand(mesh0.v.shape[0], 3, device=dev)
    out = mesh0.smooth(5)
    assert isinstance(out, MeshingResult) and out.f is mesh0.f and out.c is mesh0.c
    assert out.v.shape == mesh0.v.shape and out.v.dtype == mesh0.v.dtype and out.v.data_ptr() != mesh0.v.data_ptr()
    v, f = _np(mesh0.v), _np(mesh0.f)
    ref = G.smooth(v, f, 5)
    err, moved = np.abs(_np(out.v).astype(np.float64) - ref).max(), np.abs(_np(out.v) - v).max()
    ulp = float(np.spacing(np.float32(np.abs(v).max())))
    print('recipe mesh: V %d F %d, smoothing moved up to %.3g, max error %.3g (one ulp %.3g)' % (len(v), len(f), moved, err, ulp))
    assert moved > 1e-5 and err <= ulp
    t0, t1 = mesh0.topology(), out.topology()
    for k in ('num_edges', 'boundary_edges', 'nonmanifold_edges', 'misoriented_edges', 'invalid_faces', 'referenced_vertices'):
        assert getattr(t0, k) == getattr(t1, k), k
    assert t0.euler_characteristic == t1.euler_characteristic and t0.components().n == t1.components().n
    n = mesh0.vertex_normals()
    assert n.shape == mesh0.v.shape and n.dtype == mesh0.v.dtype
    assert np.abs(_np(n).astype(np.float64) - G.vertex_normals(v, f)).max() <= NORMAL_ATOL_F32
    ref_v = t0.vertex_ref.bool()
    centre = mesh0.v[ref_v].mean(0)
    assert bool((((mesh0.v - centre) * n).sum(1)[ref_v] > 0).all())
