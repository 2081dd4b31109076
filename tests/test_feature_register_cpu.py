"""Global registration without a GPU: the invariants of the numpy restatement (tests/feature_register_ref.py) the GPU tests compare
with, the host side of RANSAC (nksr_amd/global_register.py: drawing, edge-length test, triple fit), and the C ABI of the new entry
points."""
import ctypes as C

import numpy as np
import pytest

import feature_register_ref as fr
import register_ref


@pytest.fixture(scope='module')
def target_feature():
    d = fr.standard_inputs()
    return fr.compute_fpfh(d['target'], d['target_normal'])


def test_spfh_thirds_sum_to_the_neighbours_and_few_rows_are_undecided(target_feature):
    f = target_feature
    for g in range(3):
        assert np.array_equal(f['count'][:, 11 * g:11 * g + 11].sum(1), f['n'])
    assert f['n'].max() <= fr.MAX_NN and f['n'].mean() > 24                    # the radius holds about max_nn points
    assert np.array_equal(np.array([bin(int(m)).count('1') for m in f['mask']]), f['n'])
    share = f['undecided'].mean()
    print('undecided rows of the standard target: %.4f' % share)
    assert share <= 0.01


def test_fpfh_thirds_sum_to_200(target_feature):
    f = target_feature
    has = f['n'] > 0
    assert has.sum() > 1900
    thirds = f['data'][has].astype(np.float64).reshape(-1, 3, 11).sum(2)
    assert np.abs(thirds - 200.0).max() <= 1e-4
    assert np.all(f['data'] >= 0) and np.all(np.isfinite(f['data']))


def test_spfh_is_invariant_under_a_rigid_motion(target_feature):
    d = fr.standard_inputs()
    T = register_ref.rigid((3.0, -1.0, 2.0), 77.0, (0.3, 0.2, -0.5))
    xyz, nrm = fr.move_cloud(T, d['target'], d['target_normal'])
    f = target_feature
    d2 = ((xyz[f['idx']] - xyz[:, None]).astype(np.float64) ** 2).sum(-1).astype(np.float32)           # the same neighbours, moved
    count, n, _, und = fr.spfh(xyz, nrm, f['idx'], d2, fr.RADIUS)
    # (the moved distances are rounded anew: a neighbour within 1e-3 of the radius may change sides, its row is left out as well)
    near_edge = (np.abs(np.sqrt(f['d2'].astype(np.float64)) - fr.RADIUS) <= 1e-3 * fr.RADIUS).any(1)
    decided = ~(und | f['undecided'] | near_edge)
    assert decided.mean() > 0.9
    assert np.array_equal(count[decided], f['count'][decided]) and np.array_equal(n[decided], f['n'][decided])


def test_triple_fit_recovers_a_pose_from_three_exact_pairs():
    from nksr_amd import global_register as gr
    rs = np.random.RandomState(0)
    src = rs.randn(50, 3, 3)
    poses = [register_ref.rigid(rs.randn(3), rs.uniform(0, 180), rs.randn(3)) for _ in range(50)]
    tgt = np.stack([s @ T[:3, :3].T + T[:3, 3] for s, T in zip(src, poses)])
    fit = gr.fit_triples(src, tgt)
    assert fit.shape == (50, 3, 4)
    assert np.abs(fit - np.stack([T[:3] for T in poses])).max() <= 1e-12
    assert np.allclose(np.linalg.det(fit[:, :, :3]), 1.0)
    assert gr.fit_triples(src[:0], tgt[:0]).shape == (0, 3, 4)


def test_edge_length_test_keeps_true_triples_and_drops_a_scaled_edge():
    from nksr_amd import global_register as gr
    rs = np.random.RandomState(1)
    src = rs.randn(40, 3, 3)
    T = register_ref.rigid((1.0, 1.0, 0.0), 100.0, (1.0, 2.0, 3.0))
    tgt = src @ T[:3, :3].T + T[:3, 3]
    assert gr.edge_length_keep(src, tgt, 0.9).all()
    bad = tgt.copy()
    bad[:, 1] = bad[:, 0] + 0.8 * (bad[:, 1] - bad[:, 0])               # edge 0-1 scaled by 0.8 among the target points
    assert not gr.edge_length_keep(src, bad, 0.9).any()
    assert not gr.edge_length_keep(bad, src, 0.9).any()                 # ... and the other way round
    assert gr.edge_length_keep(src, bad, 0.0).all()


def test_drawing_is_reproducible_per_seed():
    from nksr_amd import global_register as gr
    a, ia = gr.draw_triples(500, 10000, seed=3)
    b, ib = gr.draw_triples(500, 10000, seed=3)
    c, _ = gr.draw_triples(500, 10000, seed=4)
    assert np.array_equal(a, b) and np.array_equal(ia, ib) and not np.array_equal(a[:100], c[:100])
    assert a.dtype == np.int64 and a.min() >= 0 and a.max() < 500
    assert ((a[:, 0] != a[:, 1]) & (a[:, 1] != a[:, 2]) & (a[:, 0] != a[:, 2])).all()
    assert 9900 < len(a) < 10000 and np.all(np.diff(ia) > 0) and ia.max() < 10000       # a few of 10 000 draws from 500 repeat an index
    t, i = gr.draw_triples(2, 100, seed=0)                                # two pairs: every triple repeats one
    assert t.shape == (0, 3) and i.shape == (0,)


def test_restated_ransac_finds_the_standard_pose(target_feature):
    """the whole recipe on the host, at a tenth of the draws: the pose lies inside the basin of the ICP"""
    d = fr.standard_inputs()
    fs = fr.compute_fpfh(d['source'], d['source_normal'])
    r = fr.ransac(d['source'], d['target'], fs['data'], target_feature['data'], mutual_filter=False, max_iteration=6000)
    rot, trans = register_ref.pose_error(r['transformation'], fr.T_STAR)
    print('restated RANSAC, 6000 draws: %d scored, best count %d, pose error %.4f rad, %.4f' % (r['n_scored'], r['best_count'], rot, trans))
    assert r['best_count'] >= 20 and rot < np.radians(10.0) and trans < 0.1


def test_new_entry_points_are_declared_and_bound():
    from nksr_amd import _lib
    names = ('nksr_spfh', 'nksr_fpfh', 'nksr_feature_match', 'nksr_pose_score', 'nksr_corr_accumulate')
    for name in names:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
    assert (_lib.FPFH_BINS, _lib.FPFH_MAX_K) == (33, 32) and _lib.POSE_MAX_H == 1 << 20
    assert len(_lib.lib.nksr_spfh.argtypes) == 11 and len(_lib.lib.nksr_feature_match.argtypes) == 8


def test_new_entry_points_check_their_arguments_without_a_gpu():
    from nksr_amd import _lib
    lib = _lib.lib
    lib.nksr_last_error.restype = C.c_char_p
    big = (C.c_float * 64)()
    A, Z = C.c_void_p(C.addressof(big)), None           # (never dereferenced: every call below returns first)
    f1, d1 = C.c_float(1.0), C.c_double(1.0)

    def err():
        return lib.nksr_last_error().decode()

    def each_null(fn, args):
        for k in [k for k, a in enumerate(args) if a is A]:
            bad = list(args)
            bad[k] = Z
            assert fn(*bad) != 0 and 'NULL' in err(), (fn.__name__, k, err())

    each_null(lib.nksr_spfh, [A, A, 5, A, A, 4, f1, A, A, A, Z])
    each_null(lib.nksr_fpfh, [A, A, A, 5, A, A, 4, A, Z])
    each_null(lib.nksr_feature_match, [A, 5, A, 5, A, A, A, Z])
    each_null(lib.nksr_pose_score, [A, A, 5, A, 2, d1, A, Z])
    each_null(lib.nksr_corr_accumulate, [A, A, 5, A, A, d1, A, A, Z])
    for k in (0, 33):
        assert lib.nksr_spfh(A, A, 5, A, A, k, f1, A, A, A, Z) != 0 and 'k=' in err()
        assert lib.nksr_fpfh(A, A, A, 5, A, A, k, A, Z) != 0 and 'k=' in err()
    assert lib.nksr_spfh(A, A, 5, A, A, 4, C.c_float(0.0), A, A, A, Z) != 0 and 'radius' in err()
    assert lib.nksr_feature_match(A, 1 << 31, A, 5, A, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_pose_score(A, A, 5, A, (1 << 20) + 1, d1, A, Z) != 0 and 'n_hyp' in err()
    assert lib.nksr_pose_score(A, A, 5, A, 2, C.c_double(-1.0), A, Z) != 0 and 'threshold' in err()
    assert lib.nksr_corr_accumulate(A, A, 5, A, A, C.c_double(float('nan')), A, A, Z) != 0 and 'threshold' in err()
    # nothing to do: nothing is looked at
    assert lib.nksr_spfh(Z, Z, 0, Z, Z, 4, f1, Z, Z, Z, Z) == 0
    assert lib.nksr_fpfh(Z, Z, Z, 0, Z, Z, 4, Z, Z) == 0
    assert lib.nksr_feature_match(Z, 0, Z, 5, Z, Z, Z, Z) == 0
    assert lib.nksr_pose_score(Z, Z, 5, Z, 0, d1, Z, Z) == 0
    assert lib.nksr_corr_accumulate(Z, Z, 0, Z, Z, d1, Z, Z, Z) == 0


def test_cloud_surfaces_global_registration():
    import nksr
    for name in ('compute_fpfh_feature', 'match_features', 'registration_ransac_based_on_feature_matching', 'register_global', 'FpfhFeature',
                 'RansacResult'):
        assert hasattr(nksr.cloud, name), name
    assert callable(nksr.cloud.CloudIndex.compute_fpfh_feature)
    import torch
    with pytest.raises(RuntimeError):
        nksr.cloud.compute_fpfh_feature(torch.zeros(40, 3), torch.ones(40, 3), 0.1)         # CPU tensors: refused, no fallback
