"""tests/nn_kernels_ref.py without a GPU: the references agree with oracle/network.py, the crafted inputs hold every edge they are meant
to hold, a correct fp32 evaluation in ANOTHER order passes every check of tests/test_gpu_nn_kernels.py (the bounds are not too
tight), and deliberately wrong evaluations fail them (the checks are sharp)."""
import numpy as np
import pytest

import nn_kernels_ref as R
from oracle import hierarchy, network as onet, spec

F32 = np.float32
FAMILIES = ('A', 'B')


def padded(a, extra=3):
    return np.concatenate([a, np.full((extra,) + a.shape[1:], np.nan, F32)])


def fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ---- fp32 evaluations: another order, and wrong ones ----------------------------------------------------------------------------------
def conv_eval32(case, relu, residual, mutate=None):
    """fp32, taps in reverse order, bias and residual first.  mutate: 'tap_twice' (tap 26 applied in place of tap 25), 'swap_k16'
    (input channels 3 and 19 of tap 7 swapped), 'tail_row' (row 31, the last of the first 32-tile, takes the neighbours of row n - 1)."""
    x, nbr, W = case['x'], case['nbr'].copy(), case['W'].copy()
    if mutate == 'swap_k16':
        W[7, [3, 19]] = W[7, [19, 3]]
    if mutate == 'tail_row' and case['n'] > 32:
        nbr[31] = nbr[case['n'] - 1]
    xp = np.concatenate([x, np.zeros((1, 32), F32)])
    acc = np.tile(case['b'], (case['n'], 1)).astype(F32)
    if residual:
        acc = acc + case['res']
    for s in range(26, -1, -1):
        t = 26 if (mutate == 'tap_twice' and s == 25) else s
        acc = (acc + xp[nbr[:, t]] @ W[t]).astype(F32)
    return np.maximum(acc, 0) if relu else acc


def splat_eval(ref, feat, w=None, fp64=False):
    """(sum, weight sum) over the points in reverse order: fp64 accumulators (k_splat_trilinear) or an fp32 matrix product."""
    w = ref.w32 if w is None else w
    if fp64:
        return (w[:, ::-1].astype(np.float64) @ feat[::-1].astype(np.float64)).astype(F32), w[:, ::-1].astype(np.float64).sum(1).astype(F32)
    return (w[:, ::-1] @ feat[::-1].astype(F32)).astype(F32), w[:, ::-1].sum(1, dtype=F32)


def mean_eval32(ref, feat, w=None):
    s, ws = splat_eval(ref, feat, w)
    inv = np.where(ws > 0, F32(1) / np.where(ws > 0, ws, F32(1)), F32(0)).astype(F32)
    return (s * inv[:, None]).astype(F32)


def plane_eval32(ref, normal, w=None):
    w = ref.w32 if w is None else w
    ws = w.sum(1, dtype=F32)
    inv = np.where(ws > 0, F32(1) / np.where(ws > 0, ws, F32(1)), F32(0)).astype(F32)
    out = np.zeros((len(ws), 8), F32)
    out[:, 0] = ws > 0
    out[:, 1:4] = np.einsum('vp,vpa->va', w, ref.r32).astype(F32) * inv[:, None]
    n = (w @ normal.astype(F32)).astype(F32)
    nn = np.sqrt((n * n).sum(1, dtype=F32))
    out[:, 4:7] = n * np.where(nn > F32(1e-8), F32(1) / np.where(nn > F32(1e-8), nn, F32(1)), F32(0)).astype(F32)[:, None]
    return out


@pytest.fixture(scope='module')
def clouds():
    """Per family: the crafted cloud sorted by Morton key, the oracle's two hierarchies on it and a SplatRef per (grid, level)."""
    out = {}
    for fam in FAMILIES:
        xyz, normal = R.crafted_cloud(fam)
        o = np.argsort(spec.morton_key(R.cloud_cells(xyz), 0), kind='stable')
        xs, ns = xyz[o], normal[o]
        hier = {'splatting': hierarchy.Hierarchy(R.VOXEL, 3).build_point_splatting(xs),
                'neighbourhood': hierarchy.Hierarchy(R.VOXEL, 3).build_point_neighborhood(xs)}
        refs = {(k, d): R.SplatRef(xs, h.levels[d].ijk, d, fam) for k, h in hier.items() for d in (0, 2)}
        out[fam] = dict(xyz=xyz, xs=xs, ns=ns, hier=hier, refs=refs, keys=spec.morton_key(R.cloud_cells(xs), 0))
    return out


@pytest.fixture(scope='module')
def torus():
    from nksr_amd import utils
    xyz, _ = utils.synth_torus(260, 0.32, 0.12, 0.0, 0)
    enc = hierarchy.Hierarchy(0.075, 2).build_point_splatting(xyz).levels[0]
    cand = hierarchy.Hierarchy(0.075, 2).build_point_neighborhood(xyz).levels[0]
    sel = np.random.default_rng(0).random(cand.n) > 0.3
    pruned = hierarchy.Level(cand.keys[sel], 0, 0.075)
    pruned.build_nbr()
    return enc, pruned


# ---- 1: agreement with the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
def test_conv_reference_agrees_with_the_oracle(family):
    for kind in R.CONV_KINDS:
        case = R.conv_case(129, kind, family)
        for relu in (True, False):
            got = onet.conv3(case['x'], case['nbr'], case['W'], case['b'], relu=relu)
            R.check_conv('oracle conv3', case, relu, False, padded(got))


@pytest.mark.parametrize('family', FAMILIES)
def test_splat_references_agree_with_the_oracle(clouds, family):
    c = clouds[family]
    rng = np.random.default_rng(1)
    for (kind, d), ref in c['refs'].items():
        L, vs = c['hier'][kind].levels[d], R.VOXEL * (1 << d)
        assert float(spec.inv_w0_f32(vs)) == ref.inv_w
        f32ch, f3 = R._values(rng, (len(c['xs']), 32), family), R._values(rng, (len(c['xs']), 3), family)
        ref.check_mean('oracle mean', f32ch, onet.splat(L, c['xs'], f32ch, vs, mean=True))
        s, ws = onet.splat(L, c['xs'], f3, vs, mean=False, return_weights=True)
        ref.check_sum('oracle sum', f3, s, ws)
        ref.check_plane('oracle plane', c['ns'], onet.plane_features(L, c['xs'], c['ns'], vs))
        st, en = R.site_ranges_ref(c['keys'], L.keys, d)
        cell = R.cloud_cells(c['xs'], d)
        for j in (0, L.n // 2, L.n - 1):
            assert np.array_equal(np.nonzero((cell == L.ijk[j]).all(1))[0], np.arange(st[j], en[j]))


def test_udf_reference_agrees_with_the_oracle():
    case = R.udf_case()
    hier = hierarchy.Hierarchy(R.VOXEL, 1).build_from_keys([spec.morton_key(case['ijk'], 0)])
    feat = np.zeros_like(case['feat'])
    feat[hier.levels[0].lookup(case['ijk'])] = case['feat']
    mine = R.udf_ref32(case['ijk'], case['feat'], case['xyz'], R.INV_W0, R.VOXEL)
    R.check_udf('oracle udf', mine, onet.udf_decode(hier, [feat], case['xyz']))


# ---- 2: the inputs hold their edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
def test_crafted_cloud_holds_every_edge(clouds, family):
    c = clouds[family]
    refs = c['refs']
    e = R.cloud_edges(c['xs'], c['hier']['splatting'].levels[0].ijk, refs['splatting', 0].cnt)
    R.assert_cloud_edges(e, family)
    assert any((r.cnt == 0).any() for (k, _), r in refs.items() if k == 'neighbourhood')          # voxels no point weighs at
    if family == 'A':
        assert all(r.on_plane > 0 for r in refs.values())                                       # the w <= 0 skip path, exactly on the plane
        p = c['xs'] * F32(R.INV_W0)
        assert (p * 4 == np.round(p * 4)).all()
        assert (refs['splatting', 0].cnt == 0).any()       # voxels whose only points lie ON their weight-0 planes
    for (k, d), r in refs.items():
        assert len(r.ijk) <= 2100 and (d or r.cnt.max() > 128)


def test_tables_hold_every_edge(torus):
    for n in R.CONV_N:
        holes = R.conv_case(n, 'holes', 'A')['nbr']
        assert n < 32 or 0.3 < (holes < 0).mean() < 0.5
        assert (R.conv_case(n, 'empty', 'A')['nbr'] == -1).all()
        two = R.conv_case(n, 'taps25_26', 'A')
        assert (two['nbr'][:, :25] == -1).all() and (two['nbr'][:, 25:] >= 0).all() and (two['W'][25] != two['W'][26]).any()
        assert (R.conv_case(n, 'dense', 'A')['nbr'] >= 0).all()
    W = R.conv_case(33, 'dense', 'B')['W']
    assert all((s == 13 or (W[s] != W[26 - s]).any()) and (W[s] != W[s].T).any() for s in range(27))          # asymmetric per tap
    for g in torus:
        assert (g.nbr < 0).any() and R.nbr_symmetric(g.nbr)
    assert 400 <= torus[0].n <= 900
    assert not R.nbr_symmetric(R.conv_case(33, 'dense', 'A')['nbr'])                                # (the predicate can fail)
    for n in R.WGRAD_N:
        assert (R.wgrad_case(n, 'A')['nbr'] < 0).any() or n < 8
    for cout, n in R.LINEAR_CASES:
        assert (n * cout) % 256
    assert {0, 1, 8} <= set((R.pool_case(9, 5)['end'] - R.pool_case(9, 5)['start']).tolist())
    st = {}
    case = R.udf_case()
    fresh = R.udf_ref32(case['ijk'], case['feat'], case['xyz'], R.INV_W0, R.VOXEL, stats=st)
    assert min(st.values()) > 0, st
    prev = R.udf_prev(case, fresh)
    assert ((prev < 1e29) & (prev != fresh)).any() and ((prev > 1e29) & (fresh < 1e29)).any()


# ---- 3: another order passes; 4: wrong evaluations fail ---------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
def test_conv_checks_pass_another_order_and_catch_mistakes(family):
    caught = {m: 0 for m in ('tap_twice', 'swap_k16', 'tail_row')}
    for n in R.CONV_N:
        for kind in R.CONV_KINDS:
            case = R.conv_case(n, kind, family)
            for relu, residual in R.CONV_MODES:
                R.check_conv('reversed taps', case, relu, residual, padded(conv_eval32(case, relu, residual)))
                for m in caught:
                    caught[m] += fails(R.check_conv, m, case, relu, residual, padded(conv_eval32(case, relu, residual, m)))
    assert all(v > 0 for v in caught.values()), caught
    two = R.conv_case(33, 'taps25_26', family)
    assert fails(R.check_conv, 'tap twice', two, False, False, padded(conv_eval32(two, False, False, 'tap_twice')))
    dense = R.conv_case(33, 'dense', family)
    assert fails(R.check_conv, 'tail', dense, False, False, padded(conv_eval32(dense, False, False, 'tail_row')))
    assert fails(R.check_conv, 'swap', dense, False, False, padded(conv_eval32(dense, False, False, 'swap_k16')))
    good = conv_eval32(dense, False, False)
    bad = padded(good)
    bad[33, 5] = 0.0
    assert fails(R.check_conv, 'store past n', dense, False, False, bad)


@pytest.mark.parametrize('family', FAMILIES)
def test_gradient_checks(torus, family):
    g = torus[0]
    rng = np.random.default_rng(20)
    gz, W = R._values(rng, (g.n, 32), family), R._values(rng, (27, 32, 32), family)
    gp = np.concatenate([gz, np.zeros((1, 32), F32)])
    mirrored = sum((gp[g.nbr[:, s]] @ W[26 - s].T).astype(F32) for s in range(27)).astype(F32)      # the forward kernel on mirrored taps
    R.check_dgrad('mirrored taps', family, gz, g.nbr, W, mirrored)
    unmirrored = sum((gp[g.nbr[:, s]] @ W[s].T).astype(F32) for s in range(27)).astype(F32)
    assert fails(R.check_dgrad, 'taps not mirrored', family, gz, g.nbr, W, unmirrored)
    for n in R.WGRAD_N:
        case = R.wgrad_case(n, family)
        xp = np.concatenate([case['x'], np.zeros((1, 32), F32)])
        parts = [np.stack([xp[case['nbr'][i:i + 512, s]].T @ case['gz'][i:i + 512] for s in range(27)]) for i in range(0, n, 512)]
        R.check_wgrad('chunks of 512, last first', case, sum(parts[::-1]).astype(F32))
        if n > 1:
            short = np.stack([xp[case['nbr'][:n - 1, s]].T @ case['gz'][:n - 1] for s in range(27)]).astype(F32)
            assert fails(R.check_wgrad, 'last voxel missing', case, short) or not case['gz'][n - 1].any()


@pytest.mark.parametrize('family', FAMILIES)
def test_dense_checks(family):
    for cout, n in R.LINEAR_CASES:
        case = R.linear_case(cout, n, family)
        R.check_linear('fp32', case, True, (case['x'][:, ::-1] @ case['W'][:, ::-1].T + case['b']).astype(F32))
        R.check_linear('fp32', case, False, (case['x'] @ case['W'].T).astype(F32))
        assert fails(R.check_linear, 'bias dropped', case, True, (case['x'] @ case['W'].T).astype(F32)) or not case['b'].any()
    for n in R.MLP_N:
        case = R.mlp_case(n, family)
        x = R.mlp_input(case['xyz'], case['feat'])
        h = np.maximum(x @ case['W1'].T + case['b1'], 0).astype(F32)
        out = (h[:, ::-1] @ case['W2'][:, ::-1].T + case['b2']).astype(F32)
        R.check_mlp('fp32', case, padded(out))
        spill = padded(out)
        spill[n] = out[n - 1]
        assert fails(R.check_mlp, 'row stored past n', case, spill)
        if n > 1:
            wrong = out.copy()
            wrong[n - 1] = out[n - 2]
            assert fails(R.check_mlp, 'last row from its neighbour', case, padded(wrong))
    for n_parent in (1, 9):
        for C_ in (32, 5):
            case = R.pool_case(n_parent, C_)
            sizes = (case['end'] - case['start'])
            tot = np.stack([case['child'][a:b][::-1].sum(0, dtype=F32) for a, b in zip(case['start'], case['end'])])
            R.check_pool('fp32', case, np.where(sizes[:, None] > 0, tot / np.maximum(sizes, 1)[:, None].astype(F32), F32(0)).astype(F32))
            if n_parent > 1:
                assert fails(R.check_pool, 'divided by 8', case, (tot / F32(8)).astype(F32))


@pytest.mark.parametrize('family', FAMILIES)
def test_splat_checks(clouds, family):
    c = clouds[family]
    rng = np.random.default_rng(2)
    n = len(c['xs'])
    for (kind, d), ref in c['refs'].items():
        f8, f5 = R._values(rng, (n, 8), family), R._values(rng, (n, 5), family)
        ref.check_sum('fp64 reversed', f8, *splat_eval(ref, f8, fp64=True))
        ref.check_mean('fp32 product', f5, mean_eval32(ref, f5))
        ref.check_plane('fp32', c['ns'], plane_eval32(ref, c['ns']))
    # one point dropped at a round boundary: the fifth point of a five-point cell, at one voxel it weighs at
    ref = c['refs']['splatting', 0]
    cell = R.cloud_cells(c['xs'])
    uc, first, per = np.unique(cell, axis=0, return_index=True, return_counts=True)
    k = int(first[per == 5][0]) + 4
    assert (cell[k] == cell[k - 4]).all()
    j = int(np.nonzero(ref.keep[:, k])[0][0])
    w = ref.w32.copy()
    w[j, k] = 0
    f8 = R._values(rng, (n, 8), family)
    f8[k] = 3.0
    assert fails(ref.check_sum, 'dropped', f8, *splat_eval(ref, f8, w, fp64=True))
    assert fails(ref.check_mean, 'dropped', f8, mean_eval32(ref, f8, w))
    nk = c['ns'].copy()
    nk[k] = 2.0
    assert fails(ref.check_plane, 'dropped', nk, plane_eval32(ref, nk, w))
    if family == 'A':
        # a point ON a weight-0 plane kept with weight 1e-8 and another point's feature: the voxels that only such points touch
        # are no longer empty (everywhere else fp32 absorbs 1e-8: family B may pass, the lattice's exact zeros do not)
        p = (c['xs'] * F32(ref.inv_w)).astype(F32)
        wa = F32(1) - np.abs(p[None] - (ref.ijk.astype(F32) + F32(0.5))[:, None])
        edge = (wa >= 0).all(2) & (wa == 0).any(2)
        assert edge.sum() == ref.on_plane and edge[ref.cnt == 0].any()
        w = np.where(edge, F32(1e-8), ref.w32)
        f8 = np.abs(R._values(rng, (n, 8), family)) + 1
        assert fails(ref.check_sum, 'kept', f8, *splat_eval(ref, np.roll(f8, 1, 0), w, fp64=True))
        assert fails(ref.check_mean, 'kept', f8, mean_eval32(ref, np.roll(f8, 1, 0), w))
        assert fails(ref.check_plane, 'kept', c['ns'], plane_eval32(ref, np.roll(c['ns'], 1, 0), w))


def test_udf_checks():
    case = R.udf_case()
    fresh = R.udf_ref32(case['ijk'], case['feat'], case['xyz'], R.INV_W0, R.VOXEL)
    prev = R.udf_prev(case, fresh)
    good = R.udf_ref32(case['ijk'], case['feat'], case['xyz'], R.INV_W0, R.VOXEL, only_unset=True, prev=prev)
    R.check_udf_only_unset('only_unset', case, prev, good)
    assert fails(R.check_udf_only_unset, 'only_unset ignored', case, prev, fresh)
    assert fails(R.check_udf_only_unset, 'nothing filled', case, prev, prev)
    feat = case['feat'].copy()
    feat[:, 0] = 1                                    # unoccupied voxels taken for occupied ones
    assert fails(R.check_udf, 'occupancy ignored', fresh, R.udf_ref32(case['ijk'], feat, case['xyz'], R.INV_W0, R.VOXEL))


def test_check_primitives():
    a = np.array([1.0, -2.0, 0.0], F32)
    assert R.ulp_distance(a, a).max() == 0 and R.ulp_distance(np.array([0.0], F32), np.array([-0.0], F32))[0] == 0
    assert R.ulp_distance(a, np.nextafter(a, F32(9))).tolist() == [1, 1, 1]
    assert R.bound_ratio(np.array([1.0, 0.0]), np.array([1.0, 0.0]), np.array([0.0, 0.0])) == 0.0
    assert R.bound_ratio(np.array([1.0, 1e-9]), np.array([1.0, 0.0]), np.array([1.0, 0.0])) == np.inf
    assert abs(R.gamma(866) / (866 * R.U) - 1) < 1e-4
