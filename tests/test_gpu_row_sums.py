"""The order in which the cloud tools add up their fp64 sums (csrc/icp_dev.h ``block_row_sums`` + csrc/register.hip ``k_icp_reduce``), bit
for bit.  include/nksr_hip.h promises that order; ``row_sums`` below restates it in numpy:
    rows of NKSR_ICP_BLOCK = 256 terms, the last padded with zeros; per 64 lanes the butterfly v[l] += v[l ^ o], o = 32, 16, ... 1;
    the four wavefronts of a row added in order from 0.0; then row r goes to slice r % 32, every slice adds its rows r, r + 32, ... from
    0.0, and the slices are added in order from 0.0.
The terms themselves are formed with single-rounded operations on both sides (register_ref.terms, and the plane's moments below), so the
32 sums must agree in every bit.  Sizes: one lane, the wavefront and workgroup edges, and 32 / 33 / 34 rows (the slice edge)."""
import functools

import numpy as np
import pytest
import torch

import feature_register_ref as F
import register_ref as R

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 255, 256, 257, 8192, 8193, 8455]
BLOCK, WAVE, FIELDS, SLICES = 256, 64, 32, 32


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def row_sums(terms):
    """float64 [n, 32] terms in row order -> the 32 sums in the order of the kernels"""
    n = len(terms)
    rows = (n + BLOCK - 1) // BLOCK
    v = np.zeros((rows * BLOCK, FIELDS))
    v[:n] = terms
    v = v.reshape(rows, BLOCK // WAVE, WAVE, FIELDS)
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ o]
    partial = np.zeros((rows, FIELDS))
    for w in range(BLOCK // WAVE):
        partial = partial + v[:, w, 0]
    slices = np.zeros((SLICES, FIELDS))
    for r in range(rows):
        slices[r % SLICES] = slices[r % SLICES] + partial[r]
    out = np.zeros(FIELDS)
    for k in range(SLICES):
        out = out + slices[k]
    return out


def test_the_restatement_on_small_integers():
    """(no rounding: any order gives the plain sum, and the shapes of the restatement are right)"""
    from nksr_amd import _lib
    assert (_lib.ICP_BLOCK, _lib.ICP_FIELDS) == (BLOCK, FIELDS)
    t = np.random.RandomState(0).randint(-9, 9, (8455, FIELDS)).astype(np.float64)
    assert np.array_equal(row_sums(t), t.sum(0)) and np.array_equal(row_sums(t[:1]), t[0])


# ---- plane moments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_plane_moments_add_in_the_stated_order(n):
    from nksr_amd import _lib, segment
    import segment_ref as S
    xyz = np.random.RandomState(n).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    normal = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    plane = np.concatenate([normal, [0.05]])
    res = np.abs(S.residuals(xyz, plane))
    t = float(np.median(res)) if n > 1 else float(res[0]) * 2.0         # about half of the points; the one point of n = 1
    ps = segment.PlanePass(_gpu(xyz), t)
    mask, sums = ps.run(plane)
    want_mask = res <= t
    assert np.array_equal(mask.cpu().numpy().astype(bool), want_mask) and want_mask.any()
    d = xyz.astype(np.float64) - ps.centre
    terms = np.zeros((n, FIELDS))
    terms[:, _lib.PLANE_COUNT] = 1.0
    k = _lib.PLANE_MOMENT
    for a in range(3):
        terms[:, _lib.PLANE_SUM + a] = d[:, a]
        for b in range(a, 3):
            terms[:, k] = d[:, a] * d[:, b]
            k += 1
    terms[~want_mask] = 0.0
    assert np.array_equal(_bits(sums), _bits(row_sums(terms)))
    assert sums[_lib.PLANE_COUNT] == want_mask.sum()


# ---- the ICP pass and the pass over given pairs -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _target():
    from nksr_amd import cloud
    d = R.standard_inputs()
    index = cloud.CloudIndex(_gpu(d['target']))
    return d['target'], d['normal'], index, _gpu(d['normal'])


def _source(n):
    """n points near the target's surface, in no particular order, a little off the pose"""
    target = R.standard_inputs()['target']
    rs = np.random.RandomState(1000 + n)
    near = target[rs.randint(0, len(target), n)].astype(np.float64) + rs.normal(0.0, 0.01, (n, 3))
    return R.move(np.linalg.inv(R.rigid((0.2, 1.0, 0.3), 2.0, (0.01, -0.005, 0.008))), near).astype(np.float32)


@pytest.mark.parametrize('method', ['point', 'plane'])
@pytest.mark.parametrize('n', SIZES)
def test_icp_accumulate_adds_in_the_stated_order(n, method):
    from nksr_amd import register
    target, normal, index, normal_gpu = _target()
    src, T = _source(n), np.eye(4)
    ps = register.IcpPass(index, _gpu(src), R.RADIUS, method, normal_gpu if method == 'plane' else None, T, sort_source=False)
    sums = ps.run(T)
    corr = ps.correspondences().cpu().numpy()
    assert (corr >= 0).any()
    terms = R.terms(method, R.transform(T, src), target, corr, index.bbox_centre(), normal)
    assert np.array_equal(_bits(sums), _bits(row_sums(terms)))
    assert sums[R.COUNT] == (corr >= 0).sum()


@pytest.mark.parametrize('n', SIZES)
def test_corr_accumulate_adds_in_the_stated_order(n):
    from nksr_amd import global_register as gr
    target = R.standard_inputs()['target']
    rs = np.random.RandomState(2000 + n)
    tgt = target[rs.randint(0, len(target), n)]
    T = R.rigid((0.2, 1.0, 0.3), 7.0, (0.02, -0.01, 0.015))
    src = (R.move(np.linalg.inv(T), tgt.astype(np.float64)) + rs.normal(0.0, 0.02, (n, 3))).astype(np.float32)
    centre = R.bbox_centre(tgt)
    e = np.linalg.norm(R.transform(T, src) - tgt.astype(np.float64), axis=1)
    thr = float(np.median(e)) if n > 1 else float(e[0]) * 2.0
    want_mask, terms = F.corr_terms(src, tgt, T, centre, thr)
    mask, sums = gr.corr_sums(_gpu(src), _gpu(tgt), T, centre, thr)
    assert np.array_equal(mask.cpu().numpy().astype(bool), want_mask) and want_mask.any()
    assert np.array_equal(_bits(sums), _bits(row_sums(terms)))
