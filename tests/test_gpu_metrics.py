"""MeshEvaluator on the MI355X (nksr_amd/metrics.py, csrc/metrics.hip, its k_nn_metrics on the octree search of csrc/knn_topk_dev.h) against numpy / cKDTree
restatements and the CPU oracle (oracle/metrics.py)."""
import time

import numpy as np
import pytest
import torch

import parity_util as pu

pytestmark = pytest.mark.gpu

M32 = np.uint64(0xFFFFFFFF)
# (chamfer-L1 <=, F-score@0.01 >=, normal consistency >=) of the configs[1] recipe on the analytic shapes (the quality pins' bounds)
QUALITY = {'sphere': (0.0046, 0.975, 0.985), 'torus': (0.0036, 0.985, 0.985), 'rbox': (0.0041, 0.98, 0.985)}


def _dev():
    return torch.device('cuda:0')


# ---- numpy restatement of the sampler (include/nksr_hip.h, nksr_mesh_sample) -------------------------------------------------------
def _philox(i, seed):
    i = np.asarray(i, np.uint64)
    c0, c1 = i & M32, i >> np.uint64(32)
    c2 = c3 = np.zeros_like(i)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def _sample_np(v, f, n, seed):
    """(points, face normals, faces, barycentric weights) in float64 from the float32 vertices."""
    v = np.asarray(v, np.float32).astype(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cr = np.cross(b - a, c - a)
    ln = np.linalg.norm(cr, axis=1)
    cdf = np.cumsum(0.5 * ln)
    r0, r1, r2, r3 = _philox(np.arange(n, dtype=np.uint64), seed)
    u0 = ((r0 << np.uint64(21)) ^ (r1 >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
    u1, u2 = r2.astype(np.float64) * 2.0 ** -32, r3.astype(np.float64) * 2.0 ** -32
    t = u0 * cdf[-1]
    t = np.where(t < cdf[-1], t, np.nextafter(cdf[-1], 0.0))
    j = np.searchsorted(cdf, t, side='right')
    s = np.sqrt(u1)
    w = np.stack([1.0 - s, s * (1.0 - u2), s * u2], 1)
    p = w[:, :1] * a[j] + w[:, 1:2] * b[j] + w[:, 2:] * c[j]
    nrm = cr[j] / np.maximum(ln[j], 1e-300)[:, None]
    return p, nrm, j, w


def _uv_sphere(nu=48, nv=24, r=0.4):
    th = np.linspace(0, np.pi, nv + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing='ij')
    v = np.concatenate([[[0, 0, r]], np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3),
                        [[0, 0, -r]]]).astype(np.float32)
    f = []
    idx = lambda i, k: 1 + i * nu + k % nu                                         # noqa: E731
    for k in range(nu):
        f.append([0, idx(0, k), idx(0, k + 1)])
        f.append([len(v) - 1, idx(nv - 2, k + 1), idx(nv - 2, k)])
    for i in range(nv - 2):
        for k in range(nu):
            f += [[idx(i, k), idx(i + 1, k), idx(i + 1, k + 1)], [idx(i, k), idx(i + 1, k + 1), idx(i, k + 1)]]
    return v, np.array(f, np.int64)


def test_sampler_matches_its_numpy_restatement():
    from nksr_amd import metrics
    v, f = _uv_sphere()
    n = 200000
    p, nrm, face = (x.cpu().numpy() for x in metrics.sample_surface(v, f, n, seed=7))
    pe, ne, je, _ = _sample_np(v, f, n, 7)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    perr = float(np.abs(p - pe).max()) / diag
    pu.report('metrics:sampler', face_mismatch=int((face != je).sum()), point_err_rel_diag=perr)
    assert np.array_equal(face, je)
    assert perr <= 1e-6
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-6 and np.abs(nrm - ne).max() < 1e-6
    again = [x.cpu().numpy() for x in metrics.sample_surface(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), n, seed=7)]
    assert np.array_equal(again[0], p) and np.array_equal(again[1], nrm) and np.array_equal(again[2], face)
    other = metrics.sample_surface(v, f, n, seed=8)[0].cpu().numpy()
    assert not np.array_equal(other, p)


def test_sampler_statistics_follow_the_areas():
    from scipy import stats
    from nksr_amd import metrics
    rs = np.random.RandomState(3)
    sizes = np.sqrt(2.0 * np.logspace(-4, 0, 40))                                   # areas 1e-4 .. 1
    v, f = [], []
    for k, s in enumerate(sizes):
        o = rs.uniform(-5, 5, 3)
        v += [o, o + [s, 0, 0], o + [0, s, 0]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    nz = len(f)
    for k in range(6):                                                              # zero-area triangles: collinear and repeated corners
        o = rs.randint(-5, 5, 3).astype(np.float64)                                 # (integer corners: collinear in float32 as well)
        b = len(v)
        v += [o, o + [1, 1, 1], o + [2, 2, 2]] if k % 2 else [o, o, o + [1, 0, 0]]
        f.append([b, b + 1, b + 2])
    v, f = np.array(v, np.float32), np.array(f, np.int32)
    n = 2_000_000
    p, _, face = metrics.sample_surface(v, f, n, seed=11)
    face = face.cpu().numpy()
    cnt = np.bincount(face, minlength=len(f))
    assert cnt[nz:].sum() == 0, 'a zero-area triangle was sampled'
    a = np.linalg.norm(np.cross(v[f[:nz, 1]].astype(np.float64) - v[f[:nz, 0]], v[f[:nz, 2]].astype(np.float64) - v[f[:nz, 0]]), axis=1) / 2
    chi2, pval = stats.chisquare(cnt[:nz], n * a / a.sum())
    pu.report('metrics:sampler_chi2', chi2=float(chi2), p=float(pval), min_count=int(cnt[:nz].min()))
    assert pval > 1e-3
    # barycentric coordinates of every sample in its triangle (least squares on the two edges)
    p = p.cpu().numpy().astype(np.float64)
    A, B, Cc = v[f[face, 0]].astype(np.float64), v[f[face, 1]].astype(np.float64), v[f[face, 2]].astype(np.float64)
    M = np.stack([B - A, Cc - A], 2)
    uv = np.linalg.solve(np.einsum('nki,nkj->nij', M, M), np.einsum('nki,nk->ni', M, p - A)[:, :, None])[:, :, 0]
    bary = np.concatenate([1 - uv.sum(1, keepdims=True), uv], 1)
    assert bary.min() >= -1e-4 and bary.max() <= 1 + 1e-4


def _clouds():
    rs = np.random.RandomState(5)
    uni = rs.uniform(-1, 1, (30000, 3))
    cen = rs.uniform(-1, 1, (12, 3))
    clu = np.concatenate([c + rs.normal(0, s, (2500, 3)) for c, s in zip(cen, np.logspace(-4, -1, 12))])
    dup = np.concatenate([np.repeat(rs.uniform(-1, 1, (2000, 3)), 8, axis=0), rs.uniform(-1, 1, (4000, 3))])     # 80 % exact copies
    out = {}
    for name, t in (('uniform', uni), ('clustered', clu), ('duplicates', dup)):
        t = t.astype(np.float32)
        tn = rs.normal(0, 1, t.shape).astype(np.float32)
        tn[::97] = 0.0                                                              # zero normals give a dot of 0
        ext = t.max(0) - t.min(0)
        q = np.concatenate([t[rs.randint(0, len(t), 5000)] + rs.normal(0, 0.01, (5000, 3)),   # near the cloud
                            t[rs.randint(0, len(t), 500)],                                    # on points
                            rs.uniform(-1.5, 1.5, (5000, 3)),
                            t.mean(0) + 100 * ext * rs.choice([-1, 1], (300, 3)) * rs.uniform(0.5, 1, (300, 3)),   # 100 x the bbox away
                            rs.normal(0, 1, (200, 3)) * 3e7]).astype(np.float32)             # beyond the 21-bit key range
        qn = rs.normal(0, 1, q.shape).astype(np.float32)
        out[name] = (t, tn, q, qn)
    return out


@pytest.mark.parametrize('kind', ['uniform', 'clustered', 'duplicates'])
def test_distance_p2p_is_exact(kind):
    from scipy.spatial import cKDTree
    from nksr_amd import metrics
    t, tn, q, qn = _clouds()[kind]
    dist, dot = metrics.distance_p2p(q, qn, t, tn)
    dist, dot = dist.cpu().numpy().astype(np.float64), dot.cpu().numpy().astype(np.float64)
    # the same float32 coordinates the GPU sees: recentred by the target's bounding-box centre in float64
    c = 0.5 * (t.min(0).astype(np.float64) + t.max(0).astype(np.float64))
    t32, q32 = (t - c).astype(np.float32).astype(np.float64), (q - c).astype(np.float32).astype(np.float64)
    d, i = cKDTree(t32).query(q32, k=2, workers=16)
    assert np.isfinite(dist).all(), 'a query came back without its neighbour'
    rel = np.abs(dist - d[:, 0]) / np.maximum(d[:, 0], 1e-30)
    rel[d[:, 0] == 0] = np.abs(dist[d[:, 0] == 0])
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)          # noqa: E731
    ref_dot = np.abs((unit(qn.astype(np.float64)) * unit(tn.astype(np.float64))[i[:, 0]]).sum(1))
    unique = d[:, 1] - d[:, 0] > 1e-6 * (1.0 + d[:, 0])
    assert unique.sum() > 1000
    derr = float(np.abs(dot - ref_dot)[unique].max())
    pu.report('metrics:p2p:' + kind, dist_rel=float(rel.max()), dot_abs=derr, unique=int(unique.sum()), n=len(q))
    assert rel.max() <= 1e-6
    assert derr <= 1e-6


def test_evaluate_matches_the_oracle_on_the_same_samples():
    from conftest import make_cloud
    from nksr_amd import metrics
    from oracle import metrics as om
    v, f = _uv_sphere(64, 32, 0.45)
    p, n, _ = metrics.sample_surface(v, f, 100000, seed=1)
    p, n = p.cpu().numpy(), n.cpu().numpy()
    gt, gtn = make_cloud('sphere', 60000, 0.002, 4)
    ev = metrics.MeshEvaluator(100000, metrics.MeshEvaluator.ALL_METRICS + ['f-precision-outdoor', 'f-recall-outdoor', 'f-score-outdoor'])
    m = ev.evaluate(p, gt, n, gtn)
    o = om.evaluate(p.astype(np.float64), n.astype(np.float64), gt.astype(np.float64), gtn.astype(np.float64))
    comp, _ = om.distance_p2p(gt.astype(np.float64), None, p.astype(np.float64), None)
    acc, _ = om.distance_p2p(p.astype(np.float64), None, gt.astype(np.float64), None)
    for k in ('completeness', 'accuracy', 'chamfer-L1', 'chamfer-L2', 'normals'):
        assert abs(m[k] - o[k]) <= 1e-5 * abs(o[k]), (k, m[k], o[k])
    # threshold counts: a point may only change sides when its distance lies within 1e-6 t of the threshold
    for i, t in enumerate(om.THRESHOLDS):
        bounds = []
        for key, d, cnt in (('f-precision', acc, len(p)), ('f-recall', comp, len(gt))):
            bound = int((np.abs(d - t) <= 1e-6 * t).sum())
            if i in (0, 4):
                name = key + ('-outdoor' if i == 4 else '')
                ref = float((d <= t).mean())
                assert abs(m[name] - ref) * cnt <= bound + 1e-6, (name, m[name], ref, bound)
            bounds.append(bound)
        fkey = {0: 'f-score', 1: 'f-score-15', 2: 'f-score-20', 4: 'f-score-outdoor'}.get(i)
        if fkey and bounds == [0, 0]:                                              # nothing near the threshold: the same counts
            assert abs(m[fkey] - o[fkey]) <= 1e-9, (fkey, m[fkey], o[fkey])
    pu.report('metrics:evaluate_vs_oracle', chamfer_L1=m['chamfer-L1'], d_chamfer=abs(m['chamfer-L1'] - o['chamfer-L1']),
              f_score=m['f-score'], normals=m['normals'])


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
        out[kind] = (fld.extract_dual_mesh(mise_iter=1), make_cloud(kind, 200000, 0.0, 12345))
    return out


@pytest.mark.parametrize('kind', ['sphere', 'torus', 'rbox'])
def test_eval_mesh_recipe_quality_and_oracle(kind, recipe_meshes):
    from nksr.metrics import MeshEvaluator
    from oracle import metrics as om
    mesh, (gt, gtn) = recipe_meshes[kind]
    m = MeshEvaluator(100000, MeshEvaluator.ESSENTIAL_METRICS).eval_mesh(mesh, gt, gtn)
    assert sorted(m) == sorted(MeshEvaluator.ESSENTIAL_METRICS)
    o = om.eval_mesh(mesh.v.cpu().numpy(), mesh.f.cpu().numpy(), gt, gtn, n_points=100000, seed=0)
    pu.report('metrics:eval_mesh:' + kind, chamfer_L1=m['chamfer-L1'], oracle_chamfer_L1=o['chamfer-L1'], f_score=m['f-score'],
              oracle_f_score=o['f-score'], normals=m['normals'], oracle_normals=o['normals'])
    cd, fs, nc = QUALITY[kind]
    assert m['chamfer-L1'] <= cd and m['f-score'] >= fs and m['normals'] >= nc, m
    assert abs(m['chamfer-L1'] - o['chamfer-L1']) <= 0.03 * o['chamfer-L1']
    assert abs(m['f-score'] - o['f-score']) <= 0.01 and abs(m['normals'] - o['normals']) <= 0.01


def test_eval_mesh_edge_cases(recipe_meshes):
    from nksr_amd.fields.base_field import MeshingResult
    from nksr.metrics import MeshEvaluator
    mesh, (gt, gtn) = recipe_meshes['torus']
    ev = MeshEvaluator(50000)
    empty = MeshingResult(torch.zeros((0, 3), device='cuda'), torch.zeros((0, 3), dtype=torch.int64, device='cuda'))
    m = ev.eval_mesh(empty, gt, gtn)
    assert sorted(m) == sorted(MeshEvaluator.ALL_METRICS) and all(np.isnan(x) for x in m.values())
    flat = MeshingResult(torch.zeros((3, 3), device='cuda'), torch.tensor([[0, 1, 2]], device='cuda'))
    assert all(np.isnan(x) for x in ev.eval_mesh(flat, gt, gtn).values())
    m = ev.eval_mesh(mesh, gt, None)
    for k, x in m.items():
        assert np.isnan(x) == k.startswith('normals'), (k, x)
    sub = MeshEvaluator(50000, ['f-score-outdoor', 'accuracy']).eval_mesh(mesh, gt, gtn)
    assert sorted(sub) == ['accuracy', 'f-score-outdoor']
    with pytest.raises(NotImplementedError):
        ev.eval_mesh(mesh, gt, gtn, onet_samples=[np.zeros((4, 3)), np.zeros(4)])
    full = ev.eval_mesh(mesh, gt, gtn)
    assert ev.eval_mesh(mesh, gt, gtn) == full                                      # bitwise equal run to run
    v, f = mesh.v.cpu().numpy(), mesh.f.cpu().numpy()
    m32 = ev.eval_mesh(MeshingResult(torch.from_numpy(v), torch.from_numpy(f.astype(np.int32))), gt, gtn)
    m64 = ev.eval_mesh(MeshingResult(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64))), gt, gtn)
    assert m32 == m64 == full
    off = np.array([4.5e5, 5.2e6, 0.0])
    far = ev.eval_mesh(MeshingResult(v.astype(np.float64) + off, f), gt.astype(np.float64) + off, gtn)
    for k in full:
        assert abs(far[k] - full[k]) <= 1e-5 * abs(full[k]), (k, far[k], full[k])


def test_bench_scale_scene_5m_samples():
    from scipy.spatial import cKDTree
    import nksr_amd
    from nksr_amd import metrics, utils
    dev = _dev()
    xyz, nrm = utils.synth_scene(1_000_000, seed=0)
    rec = nksr_amd.Reconstructor(dev)
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=1.0)
    mesh = fld.extract_dual_mesh(mise_iter=1)
    ev = metrics.MeshEvaluator(int(5e6), metrics.MeshEvaluator.ESSENTIAL_METRICS)
    xt, nt = torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev)
    ev.eval_mesh(mesh, xt, nt)                                                      # warm-up (allocator, code objects)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = ev.eval_mesh(mesh, xt, nt)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    assert sorted(m) == sorted(metrics.MeshEvaluator.ESSENTIAL_METRICS) and all(np.isfinite(x) for x in m.values())
    # per-query distances of a seeded subset of 2e5 queries, both directions
    s, _, _ = metrics.sample_surface(mesh.v, mesh.f, int(5e6), seed=0)
    s = s.cpu().numpy()
    rs = np.random.RandomState(0)
    errs = []
    for q, t in ((xyz[rs.choice(len(xyz), 200000, replace=False)], s), (s[rs.choice(len(s), 200000, replace=False)], xyz)):
        dist, _ = metrics.distance_p2p(q, None, t, None)
        c = 0.5 * (t.min(0).astype(np.float64) + t.max(0).astype(np.float64))
        d, _ = cKDTree((t - c).astype(np.float32)).query((q - c).astype(np.float32), workers=16)
        dist = dist.cpu().numpy().astype(np.float64)
        err = np.abs(dist - d) / np.maximum(d, 1e-30)
        err[d == 0] = dist[d == 0]
        errs.append(float(err.max()))
    pu.report('metrics:bench_scale', F=int(mesh.f.shape[0]), samples=int(5e6), eval_ms=ms, chamfer_L1=m['chamfer-L1'], f_score=m['f-score'],
              normals=m['normals'], gt_to_samples_rel=errs[0], samples_to_gt_rel=errs[1])
    assert max(errs) <= 1e-6
