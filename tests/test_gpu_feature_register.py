"""Global registration on the GPU (nksr_amd/global_register.py, csrc/fpfh.hip, csrc/global_register.hip) against the numpy restatement
(tests/feature_register_ref.py): every kernel alone on inputs both sides share -- the restatement is fed the GPU's own neighbour lists,
counts and features, so what is compared is the kernel under test and nothing before it --, then the RANSAC loop, ``register_global``
and the example.

Standard inputs: rounded box + sphere + torus, 2 000 points per cloud, the source 140 degrees and 0.86 away; FPFH radius 0.15, 32
neighbours, distance 0.03, 30 000 draws, seed 0.  The restatement alone, on the host with its own neighbour search (printed by
tests/test_feature_register_cpu.py and the figures below by the end-to-end test, -s):
    no mutual filter: 2 000 pairs, 433 of 29 962 draws scored, best holds 102 pairs, pose 0.0250 rad / 0.0213 off
    mutual filter   :   590 pairs, 483 of 29 854 draws scored, best holds  37 pairs, pose 0.1388 rad / 0.1086 off
    register_ref.icp (plane, radius 0.05) from either pose: 7.66e-4 rad / 6.04e-4 from the true pose -- the figure the GPU's pose
    after ``icp`` is held to twice of; the sampling of the two clouds differs, the error is that of the surface samples
Partial overlap (the halves of the oblique cut, band 0.15, 1 662 and 1 253 points): the restatement needs no more than 10 000 draws at
voxel 0.05 (672 / 566 points after thinning; best holds 25 of 181 mutual pairs, pose 0.105 rad / 0.087 off, ICP at 0.075 then reaches
3.5e-3 rad / 2.9e-3), so the band stays 0.15 and the test draws 30 000."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_register_ref as fr
import register_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device('cuda:0')


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)


def gpu_spfh(xyz, normal, k, radius):
    """the GPU's neighbours of ``xyz``, nksr_spfh on them, and the restatement on the same neighbours"""
    from nksr_amd import cloud, global_register as gr
    index = cloud.CloudIndex(_gpu(xyz))
    idx64, d2 = index.knn_d2(k, exclude_self=True)
    idx = idx64.to(torch.int32).contiguous()
    count, nn, mask = gr.spfh(index.xyz, _gpu(normal), idx, d2, radius)
    out = {'idx': idx, 'd2': d2, 'count': count, 'n': nn, 'mask': mask}
    out['ref'] = fr.spfh(xyz, normal, idx.cpu().numpy(), d2.cpu().numpy(), radius)
    return out


@functools.lru_cache(maxsize=None)
def std():
    """the standard clouds on the device with their features, computed once"""
    from nksr_amd import cloud
    d = fr.standard_inputs()
    out = {k: _gpu(v) for k, v in d.items()}
    for side in ('source', 'target'):
        out[side + '_spfh'] = gpu_spfh(d[side], d[side + '_normal'], fr.MAX_NN, fr.RADIUS)
        out[side + '_feature'] = cloud.compute_fpfh_feature(out[side], out[side + '_normal'], fr.RADIUS, fr.MAX_NN)
    return out


# ---- 1. SPFH -------------------------------------------------------------------------------------------------------------------------
def _check_spfh(g, what, cap=0.01):
    count, nn, mask, und = g['ref']
    share = und.mean()
    print('%s: %d rows, %.4f undecided' % (what, len(und), share))
    assert share <= cap
    ok = ~und
    assert np.array_equal(g['count'].cpu().numpy()[ok], count[ok])
    assert np.array_equal(g['n'].cpu().numpy()[ok], nn[ok])
    assert np.array_equal(g['mask'].cpu().numpy().view(np.uint32)[ok], mask[ok])
    return count, nn


@pytest.mark.parametrize('side', ['source', 'target'])
def test_spfh_counts_equal_the_restatement(side):
    count, nn = _check_spfh(std()[side + '_spfh'], side)
    assert nn.mean() > 24 and count.sum() == 3 * nn.sum()


def test_spfh_edge_shapes():
    rs = np.random.RandomState(5)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)          # noqa: E731
    # two points, one neighbour each
    g = gpu_spfh(np.array([[0.0, 0.0, 0.0], [0.1, 0.02, 0.03]], np.float32), unit(np.array([[0.0, 0.3, 1.0], [1.0, 0.2, 0.0]])), 1, 0.5)
    _, nn = _check_spfh(g, 'N = 2, k = 1', cap=0.0)
    assert nn.tolist() == [1, 1]
    # 65 points: one more than a wavefront
    g = gpu_spfh(rs.rand(65, 3).astype(np.float32), unit(rs.randn(65, 3)), 32, 0.6)
    _, nn = _check_spfh(g, 'N = 65', cap=0.0)
    assert nn.min() > 0
    # two points at one position: d2 = 0 takes no part, the other neighbours do
    xyz = rs.rand(40, 3).astype(np.float32)
    xyz[1] = xyz[0]
    g = gpu_spfh(xyz, unit(rs.randn(40, 3)), 8, 2.0)
    _, nn = _check_spfh(g, 'duplicate', cap=0.0)
    assert float(g['d2'][0, 0]) == 0.0 and float(g['d2'][1, 0]) == 0.0 and nn[0] == 7 and nn[1] == 7 and nn[2:].min() == 8
    assert not (g['mask'].cpu().numpy()[:2] & 1).any()
    # a normal parallel to d: the cross product is zero, the pair takes no part
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.125], [0.5, 0.25, 0.0]], np.float32)
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], np.float32)
    g = gpu_spfh(xyz, nrm, 2, 2.0)
    _, nn = _check_spfh(g, 'parallel normal', cap=0.0)
    assert nn.tolist() == [1, 1, 2]
    # a radius below every distance: nothing takes part, the feature is zero
    from nksr_amd import global_register as gr
    x = rs.rand(50, 3).astype(np.float32)
    g = gpu_spfh(x, unit(rs.randn(50, 3)), 8, 1e-4)
    assert int(g['count'].abs().sum()) == 0 and int(g['n'].abs().sum()) == 0 and int(g['mask'].abs().sum()) == 0
    assert float(gr.fpfh(g['count'], g['n'], g['mask'], g['idx'], g['d2']).abs().sum()) == 0.0


def test_compute_fpfh_feature_is_the_kernels_on_unit_normals():
    from nksr_amd import cloud, global_register as gr
    s = std()
    f = s['target_feature']
    assert f.data.dtype == torch.float32 and tuple(f.data.shape) == (2000, 33) and f.spfh_count.dtype == torch.int32 and f.n_neighbours.dtype == torch.int32
    index = cloud.CloudIndex(s['target'])
    f2 = index.compute_fpfh_feature(2.0 * s['target_normal'], fr.RADIUS)                # any length: scaled on the way in (a power of two: exactly)
    n = s['target_normal'].double()
    unit = (n / n.norm(dim=1, keepdim=True)).float().contiguous()
    count, nn, mask = gr.spfh(index.xyz, unit, f.neighbour_idx, f.neighbour_d2, fr.RADIUS)
    assert torch.equal(count, f.spfh_count) and torch.equal(nn, f.n_neighbours) and torch.equal(mask, f.neighbour_mask)
    assert torch.equal(f2.spfh_count, f.spfh_count) and torch.equal(f2.data, f.data)
    with pytest.raises(ValueError):
        cloud.compute_fpfh_feature(s['target'], torch.zeros_like(s['target']), fr.RADIUS)
    with pytest.raises(ValueError):
        cloud.compute_fpfh_feature(s['target'], s['target_normal'], fr.RADIUS, max_nn=33)


# ---- 2. FPFH -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['source', 'target'])
def test_fpfh_within_one_ulp_and_repeatable(side):
    from nksr_amd import global_register as gr
    g = std()[side + '_spfh']
    got = gr.fpfh(g['count'], g['n'], g['mask'], g['idx'], g['d2'])
    again = gr.fpfh(g['count'], g['n'], g['mask'], g['idx'], g['d2'])
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    want = fr.fpfh(g['count'].cpu().numpy(), g['n'].cpu().numpy(), g['mask'].cpu().numpy().view(np.uint32), g['idx'].cpu().numpy(), g['d2'].cpu().numpy())
    got = got.cpu().numpy()
    ulps = np.abs(_bits(got) - _bits(want))
    print('%s: %d of %d values differ from the restatement, at most %d ulp' % (side, int((ulps > 0).sum()), ulps.size, int(ulps.max())))
    assert np.all(np.isfinite(got)) and ulps.max() <= 1
    has = g['n'].cpu().numpy() > 0
    assert np.abs(got[has].astype(np.float64).reshape(-1, 3, 11).sum(2) - 200.0).max() <= 1e-4


# ---- 3. matching -----------------------------------------------------------------------------------------------------------------------
def _histograms(n, seed):
    """rows like the features: non-negative, every third summing to 200, many of them nearly alike"""
    rs = np.random.RandomState(seed)
    base = rs.rand(8, 3, 11) ** 4
    h = base[rs.randint(0, 8, n)] + 0.02 * rs.rand(n, 3, 11)
    return (200.0 * h / h.sum(2, keepdims=True)).reshape(n, 33).astype(np.float32)


@pytest.mark.parametrize('na,nb', [(1, 1), (63, 100), (65, 1025), (257, 64), (2000, 2000)])
def test_matching_equals_the_restatement(na, nb):
    from nksr_amd import global_register as gr
    if (na, nb) == (2000, 2000):
        s = std()
        A, B = s['source_feature'].data.cpu().numpy(), s['target_feature'].data.cpu().numpy()
    else:
        A, B = _histograms(na, 1), _histograms(nb, 2)
    idx, d2 = gr.feature_match(_gpu(A), _gpu(B))
    want_idx, want_d2 = fr.match(A, B)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(_bits(d2.cpu().numpy()), _bits(want_d2))


def test_matching_ties_zero_rows_and_rows_without_a_match():
    from nksr_amd import cloud, global_register as gr
    B0 = _histograms(300, 3)
    B = np.concatenate([B0, B0, B0[:50]])                       # every row two or three times: the lowest index wins
    A = np.concatenate([B0[::3] + np.float32(0.25), B0[:20], np.zeros((2, 33), np.float32)])
    A[5, 7], A[6, 0], A[7, 32] = np.nan, np.inf, -np.inf
    idx, d2 = gr.feature_match(_gpu(A), _gpu(B))
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    want_idx, want_d2 = fr.match(A, B)
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(d2), _bits(want_d2))
    assert idx[[5, 6, 7]].tolist() == [-1, -1, -1] and np.all(np.isinf(d2[[5, 6, 7]]))
    assert np.array_equal(idx[100:120], np.arange(20)) and np.all(d2[100:120] == 0) and idx.max() < 300
    assert idx[-1] == idx[-2] >= 0                              # an all-zero row has a nearest row like any other
    # the mutual mask, and what the filter does with it
    a, b = _histograms(257, 4), _histograms(190, 5)
    i_ab, dist, mutual = cloud.match_features(_gpu(a), _gpu(b))
    r_ab, r_d = fr.match(a, b)
    want = fr.mutual(r_ab, fr.match(b, a)[0])
    assert i_ab.dtype == torch.int64 and mutual.dtype == torch.bool and 0 < want.sum() < len(want)
    assert np.array_equal(i_ab.cpu().numpy(), r_ab) and np.array_equal(mutual.cpu().numpy(), want) and np.array_equal(_bits(dist.cpu().numpy()), _bits(r_d))
    f_ab, _, f_mutual = cloud.match_features(_gpu(a), _gpu(b), mutual_filter=True)
    assert np.array_equal(f_ab.cpu().numpy(), np.where(want, r_ab, -1)) and torch.equal(f_mutual, mutual)
    # nothing to match with, nothing to match
    idx, d2 = gr.feature_match(_gpu(a), _gpu(b[:0]))
    assert np.all(idx.cpu().numpy() == -1) and np.all(np.isinf(d2.cpu().numpy()))
    assert gr.feature_match(_gpu(a[:0]), _gpu(b))[0].numel() == 0
    huge = torch.empty((1 << 18, 33), dtype=torch.float32, device=_dev())           # 2^36 pairs: refused before any launch
    with pytest.raises(ValueError, match='voxel_downsample'):
        gr.feature_match(huge, huge)


# ---- 4. pose scoring and the sums --------------------------------------------------------------------------------------------------------
def _pairs_and_poses(c, h, seed):
    """c pairs that a pose T0 brings together up to noise, h hypotheses around T0"""
    rs = np.random.RandomState(seed)
    src = (rs.rand(c, 3) - 0.5).astype(np.float32)
    T0 = register_ref.rigid(rs.randn(3), 140.0, (0.7, -0.4, 0.3))
    tgt = (src.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3] + 0.03 * rs.randn(c, 3)).astype(np.float32)
    poses = np.stack([(register_ref.rigid(rs.randn(3), rs.uniform(0, 8), 0.03 * rs.randn(3)) @ T0)[:3] for _ in range(h)]) if h else np.zeros((0, 3, 4))
    poses[:1] = T0[:3]                                          # the first hypothesis is the pose itself
    return src, tgt, poses


@pytest.mark.parametrize('c', [3, 64, 1000, 2000])
@pytest.mark.parametrize('h', [1, 65, 129, 425])
def test_pose_scores_equal_a_numpy_count(h, c):
    from nksr_amd import global_register as gr
    src, tgt, poses = _pairs_and_poses(c, h, 100 * h + c)
    got = gr.pose_scores(_gpu(src), _gpu(tgt), poses, 0.05)
    want = fr.pose_counts(src, tgt, poses, 0.05)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert want.max() > 0 or c == 3


@pytest.mark.parametrize('h', [1, 63, 64, 65])
@pytest.mark.parametrize('c', [0, 1, 511, 512, 513])
def test_pose_scores_at_the_edges_of_the_scorer(c, h):
    """No pair, one, and one less / exactly / one more than the 2 x 256 a workgroup holds, against one transform, one less / exactly /
    one more than the 64 a workgroup stages: exact counts.  A NaN transform first, last and -- h = 65 -- alone in the last chunk: -1."""
    from nksr_amd import global_register as gr
    src, tgt, poses = _pairs_and_poses(c, h, 1000 * h + c)
    bad = sorted({0, h - 1})
    poses[bad] = np.nan
    t = 0.05
    good = np.setdiff1d(np.arange(h), bad)
    t64 = tgt.astype(np.float64)
    gap = min([np.abs(np.linalg.norm(register_ref.transform(poses[k], src) - t64, axis=1) - t).min() for k in good if c], default=1.0)
    assert gap > 1e-9                                       # no count hangs on the last bits of a distance
    want = fr.pose_counts(src, tgt, poses, t)
    got = gr.pose_scores(_gpu(src), _gpu(tgt), poses, t).cpu().numpy()
    assert np.array_equal(got, want)
    assert (want[bad] == -1).all() and (want[good] >= 0).all() and (c < 511 or h < 63 or want.max() > 0)


def test_pose_scores_of_transforms_that_are_not_finite_and_of_none():
    from nksr_amd import global_register as gr
    src, tgt, poses = _pairs_and_poses(700, 70, 9)
    poses[3, 1, 2], poses[64, 0, 3], poses[69, 2, 0] = np.nan, np.inf, -np.inf
    got = gr.pose_scores(_gpu(src), _gpu(tgt), poses, 0.05).cpu().numpy()
    assert np.array_equal(got, fr.pose_counts(src, tgt, poses, 0.05)) and got[[3, 64, 69]].tolist() == [-1, -1, -1] and got.max() > 0
    assert gr.pose_scores(_gpu(src), _gpu(tgt), poses[:0], 0.05).numel() == 0


@pytest.mark.parametrize('c', [3, 300, 2000])
def test_correspondence_sums_against_fp64(c):
    from nksr_amd import global_register as gr
    src, tgt, poses = _pairs_and_poses(c, 1, 40 + c)
    T = poses[0]
    centre = register_ref.bbox_centre(tgt)
    mask, sums = gr.corr_sums(_gpu(src), _gpu(tgt), T, centre, 0.05)
    want_mask, t = fr.corr_terms(src, tgt, T, centre, 0.05)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy().astype(bool), want_mask)
    want, scale = t.sum(0), np.abs(t).sum(0)
    rel = np.abs(sums - want) / np.maximum(scale, 1e-300)
    print('C = %d: %d inliers, worst |sum - fp64 sum| / sum |terms| = %.2e' % (c, int(want_mask.sum()), rel.max()))
    assert sums[0] == want_mask.sum() and rel.max() <= 1e-12 and np.all(sums[17:] == 0)
    again = gr.corr_sums(_gpu(src), _gpu(tgt), T, centre, 0.05)[1]
    assert np.array_equal(sums.view(np.uint64), again.view(np.uint64))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mutual_filter', [False, True])
def test_ransac_on_the_standard_inputs(mutual_filter):
    """Restatement alone on the host (module docstring): ICP from its RANSAC pose ends 7.66e-4 rad / 6.04e-4 from the true pose; the GPU's
    pose after ``icp`` must be within twice that.  Measured on one MI355X: the same draws and counts as the restatement (5 742 / 102 pairs
    without the mutual filter, 653 / 37 with it) and 7.657e-4 rad / 6.038e-4 after ``icp`` in both cases (profiles/feature_register.md)."""
    from nksr_amd import cloud
    s, d = std(), fr.standard_inputs()
    fs, ft = s['source_feature'], s['target_feature']
    res = cloud.registration_ransac_based_on_feature_matching(s['source'], s['target'], fs, ft, fr.DISTANCE, mutual_filter=mutual_filter,
                                                              max_iteration=fr.DRAWS, seed=fr.SEED)
    ref = fr.ransac(d['source'], d['target'], fs.data.cpu().numpy(), ft.data.cpu().numpy(), fr.DISTANCE, mutual_filter=mutual_filter)
    T = res.transformation.numpy()
    print('mutual_filter=%s: %d pairs, %d of %d draws scored, best draw %d holds %d pairs (restatement: draw %d, %d), pose error %.4f rad / %.4f' % (
        (mutual_filter, res.correspondence_set.shape[0], res.n_scored, res.n_drawn, res.best_hypothesis, res.best_count, ref['best_hypothesis'],
         ref['best_count']) + register_ref.pose_error(T, fr.T_STAR)))
    assert np.array_equal(res.correspondence_set.cpu().numpy(), ref['pairs'])
    assert (res.n_drawn, res.n_scored, res.best_hypothesis, res.best_count, res.refined) == (ref['n_drawn'], ref['n_scored'], ref['best_hypothesis'],
                                                                                             ref['best_count'], ref['refined'])
    assert np.abs(T - ref['transformation']).max() <= 1e-9
    ev = cloud.evaluate_registration(s['source'], s['target'], fr.DISTANCE, T)
    assert (res.fitness, res.inlier_rmse) == (ev.fitness, ev.inlier_rmse) and res.fitness > 0
    icp = cloud.icp(s['source'], s['target'], 0.05, init=T, method='plane', target_normal=s['target_normal'])
    icp_ref = register_ref.icp(d['source'], d['target'], 0.05, init=ref['transformation'], method='plane', normal=d['target_normal'])
    got, want = register_ref.pose_error(icp.transformation.numpy(), fr.T_STAR), register_ref.pose_error(icp_ref['transformation'], fr.T_STAR)
    print('after icp: %.3e rad / %.3e (restatement %.3e / %.3e)' % (got + want))
    assert got[0] <= 2.0 * want[0] and got[1] <= 2.0 * want[1]


def test_ransac_refuses_what_it_cannot_do():
    from nksr_amd import cloud
    s = std()
    fs, ft = s['source_feature'], s['target_feature']
    with pytest.raises(RuntimeError, match='fewer than ransac_n'):
        cloud.registration_ransac_based_on_feature_matching(s['source'][:2], s['target'], fs.data[:2], ft, fr.DISTANCE, mutual_filter=False)
    with pytest.raises(RuntimeError, match='survives'):           # a source shrunk tenfold: no edge lengths agree
        cloud.registration_ransac_based_on_feature_matching(0.1 * s['source'], s['target'], fs, ft, fr.DISTANCE, max_iteration=2000)
    with pytest.raises(ValueError):
        cloud.registration_ransac_based_on_feature_matching(s['source'], s['target'], fs, ft, fr.DISTANCE, ransac_n=4)


def test_register_global_on_partial_overlap():
    """Band 0.15 (module docstring: the restatement needs no more than 10 000 draws there).  The bound: the pose ICP itself reaches from
    the TRUE pose on these samples -- no start can do better --, doubled for correspondences that differ by near-ties."""
    from nksr_amd import cloud
    d = fr.partial_scans(1200, 0.15)
    g = {k: _gpu(v) for k, v in d.items()}
    res = cloud.register_global(g['source'], g['target'], 0.05, source_normal=g['source_normal'], target_normal=g['target_normal'],
                                max_iteration=30000)
    assert isinstance(res, cloud.IcpResult) and isinstance(res.ransac, cloud.RansacResult)
    floor = register_ref.pose_error(register_ref.icp(d['source'], d['target'], 0.075, init=fr.T_STAR, method='plane', normal=d['target_normal'])
                                    ['transformation'], fr.T_STAR)
    after_ransac = register_ref.pose_error(res.ransac.transformation.numpy(), fr.T_STAR)
    got = register_ref.pose_error(res.transformation.numpy(), fr.T_STAR)
    print('partial overlap: RANSAC %.4f rad / %.4f (best holds %d of %d pairs), after ICP %.3e rad / %.3e, ICP from the true pose %.3e / %.3e' % (
        after_ransac + (res.ransac.best_count, res.ransac.correspondence_set.shape[0]) + got + floor))
    assert got[0] <= 2.0 * floor[0] and got[1] <= 2.0 * floor[1]
    only = cloud.register_global(g['source'], g['target'], 0.05, source_normal=g['source_normal'], target_normal=g['target_normal'],
                                 max_iteration=30000, refine_icp=False)
    assert isinstance(only, cloud.RansacResult) and only.ransac is only
    assert np.array_equal(only.transformation.numpy(), res.ransac.transformation.numpy())          # the same call gives the same bits


def test_recons_global_registered_example(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'recons_global_registered.py'), '12000'], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    print(out.stdout)
    last = out.stdout.strip().splitlines()[-1].split()
    raw, reg = float(last[1].split('=')[1]), float(last[2].split('=')[1])
    assert (tmp_path / 'recons_global_registered.ply').exists() and reg < raw
