"""Mesh queries on the MI355X (nksr_amd/mesh_query.py, csrc/meshquery.hip) and the o3d-iou of MeshEvaluator, against the numpy
restatement of the crossing predicate and fp64 truth (tests/mesh_query_ref.py)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import mesh_query_ref as R
import parity_util as pu

pytestmark = pytest.mark.gpu

# o3d-iou floors of the configs[1] recipe meshes against the analytic occupancy of 1e5 samples (half uniform, half within N(0, 0.01)
# of the surface), measured 0.894 / 0.899 / 0.908.  Most of the misclassified samples are the near-surface half (3933 of 4367 on the
# sphere), within the reconstruction's own error of the true surface; the meshes are also open (3321 / 460 / 925 boundary edges).
IOU_FLOOR = {'sphere': 0.87, 'torus': 0.875, 'rbox': 0.885}
DIST_BOUND = 1e-6          # |d_gpu - d_fp64| / extent (fp32 corners and queries): measured <= 4e-8 on every mesh here


def _dev():
    return torch.device('cuda:0')


def _extent(v):
    v = np.asarray(v, np.float64)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def _analytic_inside(kind, p):
    p = np.asarray(p, np.float64)
    if kind == 'sphere':
        return np.linalg.norm(p, axis=1) < 0.45
    if kind == 'torus':
        return (np.hypot(p[:, 0], p[:, 1]) - 0.32) ** 2 + p[:, 2] ** 2 < 0.12 ** 2
    q = np.maximum(np.abs(p) - np.array([0.30, 0.22, 0.16]), 0.0)
    return np.linalg.norm(q, axis=1) < 0.10


def _onet_samples(kind, n, seed):
    """ONet-style samples: half uniform in the padded box [-0.55, 0.55]^3, half near the analytic surface; analytic occupancy."""
    from conftest import make_cloud
    rs = np.random.RandomState(seed)
    uni = rs.uniform(-0.55, 0.55, (n // 2, 3))
    surf, _ = make_cloud(kind, n - n // 2, 0.0, seed + 1)
    near = surf.astype(np.float64) + rs.normal(0, 0.01, surf.shape)
    p = np.concatenate([uni, near]).astype(np.float32)
    return p, _analytic_inside(kind, p)


def _queries(v, n, seed):
    """Uniform points of the padded box and points near the vertices."""
    rs = np.random.RandomState(seed)
    v = np.asarray(v, np.float64)
    lo, hi = v.min(0), v.max(0)
    pad = 0.15 * (hi - lo)
    uni = rs.uniform(lo - pad, hi + pad, (n // 2, 3))
    near = v[rs.randint(0, len(v), n - n // 2)] + rs.normal(0, 0.01 * _extent(v), (n - n // 2, 3))
    return np.concatenate([uni, near])


@pytest.fixture(scope='module')
def recipe_meshes():
    import nksr
    from conftest import make_cloud
    dev = _dev()
    out = {}
    for kind in ('sphere', 'torus', 'rbox'):
        xyz, nrm = make_cloud(kind, 3000, 0.005, 0)
        rec = nksr.Reconstructor(dev, config='snet-n3k-wnormal')
        fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=None)
        mesh = fld.extract_dual_mesh(mise_iter=1)
        v, f = mesh.v.cpu().numpy(), mesh.f.cpu().numpy().astype(np.int64)
        out[kind] = (mesh, v, f)
    return out


def _analytic_meshes():
    return {'uv_sphere': R.uv_sphere(64, 32, 0.4), 'torus': R.torus(96, 48)}


# ---- 1. per-ray crossing counts -------------------------------------------------------------------------------------------------
def test_crossing_counts_equal_the_restatement_on_voxel_and_analytic_meshes():
    from nksr_amd.mesh_query import MeshQuery
    rows = []
    cases = {k: R.voxel_mesh(s, i) + (s,) for i, (k, s) in enumerate(sorted(R.voxel_sets().items()))}
    for name, (v, f, vox) in cases.items():
        q, _ = R.voxel_queries(vox, v, f)
        rows.append((name, v, f, q, 7))
    for name, (v, f) in _analytic_meshes().items():
        rows.append((name, v, f, _queries(v, 600, 1), 3))
    for name, v, f, q, rays in rows:
        got = MeshQuery(v, f).crossings(q, rays=rays).cpu().numpy()
        v32, q32 = R.recentre(v, q)
        ref = R.crossings(v32, f, q32, rays)
        pu.report('mesh_query:crossings:' + name, queries=len(q), rays=rays, faces=len(f), mismatched=int((got != ref).sum()),
                  max_count=int(ref.max()))
        assert np.array_equal(got, ref), name


@pytest.mark.parametrize('kind', ['sphere', 'torus', 'rbox'])
def test_crossing_counts_equal_the_restatement_on_recipe_meshes(kind, recipe_meshes):
    from nksr_amd.mesh_query import MeshQuery
    _, v, f = recipe_meshes[kind]
    q = _queries(v, 400, 2)
    got = MeshQuery(v, f).crossings(q, rays=3).cpu().numpy()
    v32, q32 = R.recentre(v, q)
    ref = R.crossings(v32, f, q32, 3)
    pu.report('mesh_query:crossings:recipe_' + kind, queries=len(q), faces=len(f), mismatched=int((got != ref).sum()))
    assert np.array_equal(got, ref)


# ---- 2. occupancy against truth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['blob', 'pocket', 'shell', 'stairs'])
def test_occupancy_is_exact_on_voxel_unions(kind):
    from nksr_amd.mesh_query import MeshQuery
    vox = R.voxel_sets()[kind]
    v, f = R.voxel_mesh(vox, 3)
    q, inside = R.voxel_queries(vox, v, f)
    mq = MeshQuery(v, f)
    for rays in (1, 3):
        occ = mq.occupancy(q, rays=rays).cpu().numpy()
        assert np.array_equal(occ, inside), (kind, rays, int((occ != inside).sum()))


@pytest.mark.parametrize('name', ['uv_sphere', 'torus', 'convex'])
def test_occupancy_equals_the_winding_number_off_the_surface(name):
    from nksr_amd.mesh_query import MeshQuery
    if name == 'convex':
        v, f, _, _ = R.convex_polyhedron(60, 3, 0.45)
    else:
        v, f = _analytic_meshes()[name]
    q = _queries(v, 4000, 3)
    d, _ = R.distance_bruteforce(v, f, q)
    keep = d > 1e-5 * _extent(v)
    w = R.winding_number(v, f, q)
    truth = np.abs(w) > 0.5
    mq = MeshQuery(v, f)
    for rays in (1, 3, 7):
        occ = mq.occupancy(q, rays=rays).cpu().numpy()
        bad = int((occ != truth)[keep].sum())
        pu.report('mesh_query:occupancy_vs_winding:%s:rays%d' % (name, rays), queries=int(keep.sum()), inside=int(truth[keep].sum()),
                  mismatched=bad)
        assert bad == 0


# ---- 3. invariances --------------------------------------------------------------------------------------------------------------
def test_occupancy_invariances(recipe_meshes):
    from nksr_amd.mesh_query import MeshQuery
    _, v, f = recipe_meshes['torus']
    p, _ = _onet_samples('torus', 20000, 5)
    dev = _dev()
    base = MeshQuery(v, f).occupancy(p, rays=3).cpu().numpy()
    assert 1000 < base.sum() < len(base) - 1000
    rs = np.random.RandomState(0)
    perm = rs.permutation(len(f))
    variants = {
        'flipped': MeshQuery(v, f[:, ::-1].copy()).occupancy(p, rays=3),
        'permuted': MeshQuery(v, f[perm]).occupancy(p, rays=3),
        'int32': MeshQuery(v, f.astype(np.int32)).occupancy(p, rays=3),
        'cpu_tensors': MeshQuery(torch.from_numpy(v), torch.from_numpy(f)).occupancy(torch.from_numpy(p), rays=3),
        'gpu_tensors': MeshQuery(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)).occupancy(torch.from_numpy(p).to(dev), rays=3),
        'again': MeshQuery(v, f).occupancy(p, rays=3),
    }
    for k, occ in variants.items():
        assert occ.dtype == torch.bool and occ.is_cuda
        assert np.array_equal(occ.cpu().numpy(), base), k
    # far from the origin: the same answers away from the surface (the recentring happens in float64)
    off = np.array([4.5e5, 5.2e6, 0.0])
    d, _ = MeshQuery(v, f).distance(p)
    away = d.cpu().numpy() > 1e-4 * _extent(v)
    far = MeshQuery(v.astype(np.float64) + off, f).occupancy(p.astype(np.float64) + off, rays=3).cpu().numpy()
    assert np.array_equal(far[away], base[away])
    # the tree is the same bit for bit from one build to the next
    a, b = MeshQuery(v, f), MeshQuery(v, f)
    bits = lambda t: t.view(torch.int32)                                            # noqa: E731  (child words are NaN as floats)
    assert torch.equal(bits(a.bvh.nodes), bits(b.bvh.nodes)) and torch.equal(bits(a.bvh.leaves), bits(b.bvh.leaves))
    assert a.depth == b.depth
    pu.report('mesh_query:invariances', faces=len(f), queries=len(p), depth=a.depth, away=int(away.sum()))


def test_one_mesh_in_every_input_form():
    """The unit cube far from the origin (every coordinate exact in float32) as numpy arrays, CPU tensors and GPU tensors, with int32
    and int64 faces: MeshQuery, MeshTopology and sample_surface answer bit for bit alike.  Faces stored as floating point are read
    by MeshQuery and sample_surface and refused by MeshTopology (the two readers of nksr_amd/mesh_input.py)."""
    from nksr_amd.mesh_query import MeshQuery
    from nksr_amd.mesh_topology import MeshTopology
    from nksr_amd.metrics import sample_surface
    dev = _dev()
    off = np.array([1048576.0, -2097152.0, 4194304.0])
    v = np.array([[i & 1, i >> 1 & 1, i >> 2] for i in range(8)], np.float64) + off
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 7, 3], [2, 6, 7], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]],
                 np.int64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    c = v - off
    assert np.einsum('ij,ij->', c[f[:, 0]], np.cross(c[f[:, 1]], c[f[:, 2]])) / 6.0 == 1.0        # outward: the signed volume
    u = np.random.RandomState(7).uniform(-0.5, 1.5, (64, 3))
    q = u + off                                                                     # float64 in every form: float32 has no such points
    inside = np.all((u > 0) & (u < 1), axis=1)
    assert 2 < inside.sum() < 62
    forms = {'numpy_f64_i64': (v, f, q),
             'cpu_f32_i32': (torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.astype(np.int32)), torch.from_numpy(q)),
             'gpu_f32_i64': (torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(q).to(dev))}
    forms['float_faces'] = (v, f.astype(np.float64), q)

    def answers(vv, ff, qq):
        mq = MeshQuery(vv, ff)
        d, face = mq.distance(qq)
        return (d, face, mq.occupancy(qq, rays=3), mq.signed_distance(qq)) + sample_surface(vv, ff, n=256, seed=7)
    names = ('distance', 'face', 'occupancy', 'signed_distance', 'sample points', 'sample normals', 'sample faces')
    base = answers(*forms['numpy_f64_i64'])
    assert np.array_equal(base[2].cpu().numpy(), inside)
    assert base[4].dtype == torch.float32 and base[6].dtype == torch.int64 and int(base[6].min()) >= 0 and int(base[6].max()) < 12
    for form, args in forms.items():
        for name, a, b in zip(names, answers(*args), base):
            assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, (form, name)
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (form, name)
    for form in ('numpy_f64_i64', 'cpu_f32_i32', 'gpu_f32_i64'):
        t = MeshTopology(*forms[form][:2])
        totals = (t.num_edges, t.boundary_edges, t.nonmanifold_edges, t.misoriented_edges, t.invalid_faces, t.referenced_vertices)
        assert totals == (18, 0, 0, 0, 0, 8) and t.euler_characteristic == 2, (form, totals)
    with pytest.raises(ValueError, match='expected integer indices'):
        MeshTopology(v, f.astype(np.float64))


# ---- 4. distance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['sphere', 'torus', 'rbox'])
def test_distance_against_the_fp64_brute_force(kind, recipe_meshes):
    from nksr_amd.mesh_query import MeshQuery
    _, v, f = recipe_meshes[kind]
    q = _queries(v, 1500, 4)
    mq = MeshQuery(v, f)
    d, face, cp = mq.distance(q, closest_point=True)
    d, face, cp = d.cpu().numpy().astype(np.float64), face.cpu().numpy(), cp.cpu().numpy().astype(np.float64)
    assert face.dtype == np.int64 and cp.shape == (len(q), 3)
    # truth on the float32 coordinates the GPU sees (recentred), shifted back
    v32, q32 = R.recentre(v, q)
    two, ref_face = R.distance_two_best(v32, f, q32)
    ext = _extent(v)
    err = float(np.abs(d - two[:, 0]).max()) / ext
    gap = (two[:, 1] - two[:, 0]) > 2 * DIST_BOUND * ext
    cp_err = float(np.abs(np.linalg.norm(cp - q, axis=1) - two[:, 0]).max()) / ext
    pu.report('mesh_query:distance:' + kind, faces=len(f), queries=len(q), err_rel_extent=err, closest_point_err=cp_err,
              unique=int(gap.sum()), face_mismatch=int((face != ref_face)[gap].sum()))
    assert err <= DIST_BOUND
    assert np.array_equal(face[gap], ref_face[gap]) and gap.sum() > 300          # (a query nearest to a shared vertex or edge ties)
    assert cp_err <= 4 * DIST_BOUND
    sd = mq.signed_distance(q, rays=3).cpu().numpy()
    occ = mq.occupancy(q, rays=3).cpu().numpy()
    assert np.array_equal(np.abs(sd), d.astype(np.float32)) and np.array_equal(sd[d > 0] < 0, occ[d > 0])


def test_empty_mesh_and_errors():
    from nksr_amd import _lib
    from nksr_amd.mesh_query import MeshQuery, mesh_occupancy
    q = np.random.RandomState(0).uniform(-1, 1, (100, 3))
    e = MeshQuery(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    assert not e.occupancy(q).any()
    d, face = e.distance(q)
    assert torch.isinf(d).all() and (face == -1).all()
    v, f = R.uv_sphere(16, 8)
    mq = MeshQuery(v, f)
    for rays in (0, 2, 4, 9):
        with pytest.raises(ValueError):
            mq.occupancy(q, rays=rays)
        with pytest.raises(ValueError):
            mq.signed_distance(q, rays=rays)
    for bad in (np.zeros((5, 2)), np.zeros((5, 3, 1)), np.array([[0.0, np.nan, 0.0]]), np.array([[np.inf, 0.0, 0.0]])):
        with pytest.raises(ValueError):
            mq.occupancy(bad)
        with pytest.raises(ValueError):
            mq.distance(bad)
    with pytest.raises(ValueError):
        MeshQuery(v, f + 1000)
    with pytest.raises(ValueError):
        MeshQuery(v, f[:, :2])
    with pytest.raises(ValueError):
        MeshQuery(v[:, :2], f)
    with pytest.raises(ValueError):
        mesh_occupancy(v, f, q, rays=2)
    # the ABI answers NKSR_ERR_ARG for an even ray count on a real tree, and NKSR_ERR_CAPACITY for a tree deeper than the stack
    qt = torch.zeros((4, 3), device=_dev())
    out = torch.zeros(4, dtype=torch.uint8, device=_dev())
    assert _lib.lib.nksr_mesh_occupancy(C.byref(mq.bvh.struct), qt.data_ptr(), 4, None, 2, out.data_ptr(), None, None) == -1
    st = _lib.BvhT.from_buffer_copy(mq.bvh.struct)
    st.depth = _lib.BVH_STACK + 1
    assert _lib.lib.nksr_mesh_occupancy(C.byref(st), qt.data_ptr(), 4, None, 3, out.data_ptr(), None, None) == -3


def test_a_tree_deeper_than_the_stack_is_refused(monkeypatch):
    from nksr_amd import mesh_query
    v, f = R.uv_sphere(16, 8)
    depth = mesh_query.MeshQuery(v, f).depth
    assert 0 < depth <= mesh_query.BVH_STACK
    monkeypatch.setattr(mesh_query, 'BVH_STACK', depth - 1)
    with pytest.raises(RuntimeError):
        mesh_query.MeshQuery(v, f)


# ---- 5. o3d-iou -------------------------------------------------------------------------------------------------------------------
def test_eval_mesh_iou_is_the_formula_on_mesh_query(recipe_meshes):
    from nksr_amd import mesh_input, metrics
    from nksr_amd.fields.base_field import MeshingResult
    from nksr.metrics import MeshEvaluator
    from conftest import make_cloud
    mesh, v, f = recipe_meshes['sphere']
    gt, gtn = make_cloud('sphere', 100000, 0.0, 12345)
    p, occ = _onet_samples('sphere', 30000, 9)
    ev = MeshEvaluator(50000, ['chamfer-L1', 'o3d-iou'])
    m = ev.eval_mesh(mesh, gt, gtn, onet_samples=[p, occ])
    assert sorted(m) == ['chamfer-L1', 'o3d-iou']
    # the same frame as eval_mesh: everything recentred by the target's box centre
    c = mesh_input.bbox_centre(gt)
    v32 = mesh_input.recentre(mesh.v, c, _dev(), 'v')
    ff = mesh_input.faces(mesh.f, v32.shape[0], _dev(), cast_float=True, check_range=True)
    pd = metrics.MeshQuery.recentred(v32, ff, c).occupancy(p, rays=3).cpu().numpy()
    ref = np.sum(pd & occ) / (np.sum(pd | occ) + 1e-6)
    assert m['o3d-iou'] == ref
    self_iou = ev.eval_mesh(mesh, gt, gtn, onet_samples=(torch.from_numpy(p), torch.from_numpy(pd.astype(np.float32))))['o3d-iou']
    assert abs(self_iou - 1.0) <= 1e-9 and self_iou == pd.sum() / (pd.sum() + 1e-6)
    empty = MeshingResult(torch.zeros((0, 3), device='cuda'), torch.zeros((0, 3), dtype=torch.int64, device='cuda'))
    assert np.isnan(ev.eval_mesh(empty, gt, gtn, onet_samples=[p, occ])['o3d-iou'])
    with pytest.raises(ValueError):
        ev.eval_mesh(mesh, gt, gtn)
    with pytest.raises(NotImplementedError, match='metric_names'):
        MeshEvaluator(50000).eval_mesh(mesh, gt, gtn, onet_samples=[p, occ])
    assert ev.eval_mesh(mesh, gt, gtn, onet_samples=[p, occ]) == m                   # bitwise equal run to run


@pytest.mark.parametrize('kind', ['sphere', 'torus', 'rbox'])
def test_eval_mesh_iou_of_the_recipe(kind, recipe_meshes):
    from nksr.metrics import MeshEvaluator
    from conftest import make_cloud
    mesh, v, f = recipe_meshes[kind]
    gt, gtn = make_cloud(kind, 100000, 0.0, 12345)
    p, occ = _onet_samples(kind, 100000, 11)
    from nksr_amd.mesh_query import MeshQuery
    m = MeshEvaluator(100000, MeshEvaluator.ESSENTIAL_METRICS + ['o3d-iou']).eval_mesh(mesh, gt, gtn, onet_samples=[p, occ])
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    mq = MeshQuery(v, f)
    iou = {}
    for rays in (1, 7):
        pd = mq.occupancy(p, rays=rays).cpu().numpy()
        iou[rays] = float(np.sum(pd & occ) / (np.sum(pd | occ) + 1e-6))
    pd = mq.occupancy(p, rays=3).cpu().numpy()
    half = len(p) // 2
    pu.report('mesh_query:iou:' + kind, iou=m['o3d-iou'], floor=IOU_FLOOR[kind], iou_rays1=iou[1], iou_rays7=iou[7],
              wrong_uniform=int((pd != occ)[:half].sum()), wrong_near=int((pd != occ)[half:].sum()), boundary_edges=int((cnt == 1).sum()),
              chamfer_L1=m['chamfer-L1'], inside=int(occ.sum()))
    assert m['o3d-iou'] >= IOU_FLOOR[kind]


# ---- 6. scale --------------------------------------------------------------------------------------------------------------------
def test_scale_scene_mesh_1m_queries():
    import nksr_amd
    from nksr_amd import mesh_query, utils
    dev = _dev()
    xyz, nrm = utils.synth_scene(1_000_000, seed=0)
    rec = nksr_amd.Reconstructor(dev)
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=1.0)
    mesh = fld.extract_dual_mesh(mise_iter=1)
    v, f = mesh.v, mesh.f
    q = torch.from_numpy(_queries(xyz[::50], 1_000_000, 6)).to(dev)
    mesh_query.MeshQuery(v, f).occupancy(q[:1000])                                  # warm-up
    times = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times[name] = 1e3 * (time.perf_counter() - t0)
        return out
    mq = timed('build_ms', lambda: mesh_query.MeshQuery(v, f))
    occ1 = timed('occupancy_rays1_ms', lambda: mq.occupancy(q, rays=1))
    occ3 = timed('occupancy_rays3_ms', lambda: mq.occupancy(q, rays=3))
    d, face = timed("distance_ms", lambda: mq.distance(q))
    assert torch.isfinite(d).all() and (face >= 0).all()
    vn, fn, qn = v.cpu().numpy(), f.cpu().numpy().astype(np.int64), q.cpu().numpy()
    v32, q32 = R.recentre(vn, qn)
    rs = np.random.RandomState(0)
    sub = rs.choice(len(qn), 64, replace=False)
    ref = R.crossings(v32, fn, q32[sub], 3)
    got = mq.crossings(q[torch.from_numpy(sub).to(dev)], rays=3).cpu().numpy()
    assert np.array_equal(got, ref)
    assert np.array_equal(occ3.cpu().numpy()[sub], R.occupancy_from_counts(ref))
    assert np.array_equal(occ1.cpu().numpy()[sub], ref[:, 0] % 2 == 1)
    sub = rs.choice(len(qn), 256, replace=False)
    ext = _extent(vn)
    dg = d.cpu().numpy()[sub].astype(np.float64)
    dr, _ = R.distance_bruteforce(v32, fn, q32[sub], upper=dg, margin=1e-3 * ext)
    err = float(np.abs(dg - dr).max()) / ext
    pu.report('mesh_query:scale', faces=len(fn), queries=len(qn), depth=mq.depth, dist_err_rel_extent=err, inside=int(occ3.sum()),
              **times)
    assert err <= DIST_BOUND
