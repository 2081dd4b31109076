"""Every sparse-network kernel alone (csrc/nn.hip, the splats of csrc/splat.hip with splat_for_each_point of csrc/common.h)
against the exact and fp64 references of tests/nn_kernels_ref.py, which tests/test_nn_kernels_ref_cpu.py verifies without a GPU.

Family A inputs sit on a lattice where every fp32 sum is exact: those comparisons are bit for bit (2 ulp behind a division or a square
root).  Family B inputs are random fp32 and are held to the componentwise bound gamma(m) sum |terms| (m from the operation count, see
the reference module); the measured error / bound is printed by parity_util.check.  The kernels are reached the way production
reaches them (nksr_amd.nn.network, nksr_amd.nn.backward), through _lib.call where only the C entry exists."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import nn_kernels_ref as R
import parity_util as pu

pytestmark = pytest.mark.gpu

FAMILIES = ('A', 'B')


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def nan_padded(n, C_, extra=3):
    """A NaN-filled buffer and its first n rows as the kernel's `out` (same start, so `out` keeps the buffer's 16-byte alignment)."""
    buf = torch.full((n + extra, C_), float('nan'), dtype=torch.float32, device='cuda')
    return buf, buf[:n]


def call(name, *args):
    from nksr_amd._lib import call as c
    c(name, *args)


def stream():
    from nksr_amd._lib import stream as s
    return s()


def ptr(t):
    from nksr_amd._lib import ptr as p
    return p(t)


# ---- convolution --------------------------------------------------------------------------------------------------------------------
def _conv_module(case):
    from nksr_amd.nn.network import SparseConv3
    m = SparseConv3(32)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(case['W']))
        m.bias.copy_(torch.from_numpy(case['b']))
    return m.cuda()


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('n', R.CONV_N)
def test_sparse_conv3(n, family):
    """Hand-made neighbour tables (dense, 40 % missing, all missing = the bias, only taps 25 and 26), relu on / off, residual present /
    absent, asymmetric weights; the module's forward and a direct call into a NaN-padded buffer are bit-identical."""
    worst = 0.0

    def keep(name, measured, bound):
        nonlocal worst
        worst = max(worst, measured)
        assert measured <= bound, '%s: measured %.3e > bound %.3e' % (name, measured, bound)

    for kind in R.CONV_KINDS:
        case = R.conv_case(n, kind, family)
        m = _conv_module(case)
        x, nbr, res = dev(case['x']), dev(case['nbr']), dev(case['res'])
        W, b = m.weight.detach().contiguous(), m.bias.detach().contiguous()
        for relu, residual in R.CONV_MODES:
            name = 'conv3:%s:n=%d:%s:relu=%d:res=%d' % (family, n, kind, relu, residual)
            buf, out = nan_padded(n, 32)
            call('nksr_sparse_conv3', ptr(x), ptr(nbr), n, 32, ptr(W), ptr(b), ptr(res) if residual else None, int(relu), out.data_ptr(), stream())
            R.check_conv(name, case, relu, residual, host(buf), keep)
            again = m(x, nbr, relu=relu, residual=res if residual else None)
            assert torch.equal(again, out), name + ': two runs differ'
            if kind == 'empty' and not residual:
                bias = np.maximum(case['b'], 0) if relu else case['b']
                R.check_exact(name + ':bias', host(out), np.tile(bias, (n, 1)))
    if family == 'B':
        pu.check('conv3:B:n=%d' % n, worst, 1.0)


@functools.lru_cache(None)
def _torus_grids():
    """Level 0 of the point-splatting hierarchy of a small torus, and a pruned decoder (neighbourhood) grid."""
    from nksr_amd import utils
    from nksr_amd.svh import SparseFeatureHierarchy, SparseGrid
    xyz, _ = utils.synth_torus(260, 0.32, 0.12, 0.0, 0)
    pts = torch.from_numpy(xyz).cuda()
    enc = SparseFeatureHierarchy(0.075, 2, 'cuda').build_point_splatting(pts).level(0)
    cand = SparseFeatureHierarchy(0.075, 2, 'cuda').build_point_neighborhood(pts).level(0)
    sel = torch.from_numpy(np.random.default_rng(0).random(cand.num_voxels) > 0.3).cuda()
    pruned = SparseGrid(cand.keys[sel].contiguous(), 0, 0.075)
    return enc, pruned


def test_neighbour_tables_are_symmetric():
    for g in _torus_grids():
        nbr = host(g.nbr)
        assert (nbr < 0).any() and (nbr[:, 13] == np.arange(len(nbr))).all()
        assert R.nbr_symmetric(nbr)


@pytest.mark.parametrize('family', FAMILIES)
def test_conv3_dgrad(family):
    """The mirrored-tap data gradient on a real grid with missing neighbours against the fp64 transpose of the forward reference."""
    from nksr_amd.nn.backward import conv3_dgrad
    g = _torus_grids()[0]
    nbr = host(g.nbr)
    n = len(nbr)
    assert 400 <= n <= 900 and (nbr < 0).any(), n
    rng = np.random.default_rng(20)
    gz, W = R._values(rng, (n, 32), family), R._values(rng, (27, 32, 32), family)
    got = host(conv3_dgrad(dev(gz), g.nbr, dev(W)))
    R.check_dgrad('dgrad:%s:n=%d' % (family, n), family, gz, nbr, W, got, pu.check)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('n', R.WGRAD_N)
def test_conv3_wgrad(n, family):
    from nksr_amd._lib import lib
    from nksr_amd.nn.backward import conv3_wgrad
    assert int(lib.nksr_conv3_wgrad_chunks(n)) == -(-n // R.WGRAD_CHUNK)
    case = R.wgrad_case(n, family)
    got = conv3_wgrad(dev(case['x']), dev(case['nbr']), dev(case['gz']))
    assert got.shape == (27, 32, 32)
    R.check_wgrad('wgrad:%s:n=%d' % (family, n), case, host(got), pu.check)


# ---- linear head, pooling, gathers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cout,n', R.LINEAR_CASES)
def test_linear(cout, n, family):
    from nksr_amd.nn.network import Head
    assert (n * cout) % 256
    case = R.linear_case(cout, n, family)
    head = Head(32, cout, 1.0)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(case['W']))
        head.bias.copy_(torch.from_numpy(case['b']))
    head = head.cuda()
    x = dev(case['x'])
    name = 'linear:%s:Cout=%d:n=%d' % (family, cout, n)
    R.check_linear(name + ':bias', case, True, host(head(x)), pu.check)
    out = torch.full((n, cout), float('nan'), dtype=torch.float32, device='cuda')
    call('nksr_linear', ptr(x), n, 32, ptr(head.weight.detach().contiguous()), None, cout, ptr(out), stream())
    R.check_linear(name + ':no bias', case, False, host(out), pu.check)


@pytest.mark.parametrize('C_', (32, 5))
@pytest.mark.parametrize('n_parent', (1, 9))
def test_pool_children(n_parent, C_):
    case = R.pool_case(n_parent, C_)
    buf, out = nan_padded(n_parent, C_)
    child, start, end = dev(case['child']), dev(case['start']), dev(case['end'])
    call('nksr_pool_children', ptr(child), ptr(start), ptr(end), n_parent, C_, out.data_ptr(), stream())
    assert torch.isnan(buf[n_parent:]).all()
    R.check_pool('pool:parents=%d:C=%d' % (n_parent, C_), case, host(out))


@pytest.mark.parametrize('n', (1, 7, 8, 9, 33))
def test_gather_rows(n):
    """The 16-byte path (C = 32, aligned) and the generic kernel (C = 3, 8, and C = 32 through a source view offset by one float): equal
    to the torch expression bit for bit, and to each other."""
    from nksr_amd.nn.network import gather_rows
    rng = np.random.default_rng(n)
    for C_ in (32, 3, 8):
        rows = n + 2
        src = dev(rng.standard_normal((rows, C_)), np.float32)
        idx = rng.integers(-1, rows, size=n).astype(np.int32)
        idx[0] = -1 if n > 1 else 0
        add = dev(rng.standard_normal((n, C_)), np.float32)
        idx_d = dev(idx)
        want = torch.where((idx_d >= 0)[:, None], src[idx_d.clamp_min(0).long()], torch.zeros((), device='cuda'))
        for a, w in ((None, want), (add, want + add)):
            got = gather_rows(src, idx_d, add=a)
            assert torch.equal(got, w), (n, C_, a is not None)
            if C_ == 32:
                shifted = torch.empty(rows * 32 + 1, dtype=torch.float32, device='cuda')[1:].view(rows, 32)
                shifted.copy_(src)
                assert shifted.data_ptr() % 16 == 4 and src.data_ptr() % 16 == 0
                assert torch.equal(gather_rows(shifted, idx_d, add=a), got), (n, a is not None)
    none = gather_rows(src, torch.full((n,), -1, dtype=torch.int32, device='cuda'))
    assert not none.any()


# ---- point MLP ---------------------------------------------------------------------------------------------------------------------
def _mlp_direct(case, xyz=None, feat=None):
    xyz = dev(case['xyz']) if xyz is None else xyz
    feat = dev(case['feat']) if feat is None else feat
    n = xyz.shape[0]
    buf, out = nan_padded(n, 32)
    W1, b1, W2, b2 = (dev(case[k]) for k in ('W1', 'b1', 'W2', 'b2'))
    call('nksr_point_mlp', ptr(xyz), ptr(feat), n, R.INV_W0, 32, ptr(W1), ptr(b1), ptr(W2), ptr(b2), out.data_ptr(), stream())
    return buf, out


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('n', R.MLP_N)
def test_point_mlp(n, family):
    case = R.mlp_case(n, family)
    assert n == 1 or (case['xyz'][0] < 0).all()
    buf, _ = _mlp_direct(case)
    R.check_mlp('point_mlp:%s:n=%d' % (family, n), case, host(buf), pu.check)


# ---- splats ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _cloud(family):
    """The crafted cloud through sort_cloud, both hierarchies on it, and one SplatRef per (grid, level): shared, never modified."""
    from nksr_amd.nn.network import sort_cloud
    from nksr_amd.svh import SparseFeatureHierarchy
    xyz, normal = R.crafted_cloud(family)
    ks, xs, ns = sort_cloud(dev(xyz), dev(normal), R.INV_W0)
    keys = R.spec.morton_key(R.cloud_cells(host(xs)), 0)
    assert np.array_equal(host(ks), keys) and (np.diff(keys) >= 0).all()
    both = lambda p, q: np.concatenate([p, q], 1)
    assert np.array_equal(np.sort(both(host(xs), host(ns)).view('f4,f4,f4,f4,f4,f4'), axis=0), np.sort(both(xyz, normal).view('f4,f4,f4,f4,f4,f4'), axis=0))
    svh = {'splatting': SparseFeatureHierarchy(R.VOXEL, 3, 'cuda').build_point_splatting(xs),
           'neighbourhood': SparseFeatureHierarchy(R.VOXEL, 3, 'cuda').build_point_neighborhood(xs)}
    assert svh['splatting'].inv_w0 == R.INV_W0
    refs = {(kind, d): R.SplatRef(host(xs), host(h.level(d).ijk), d, family) for kind, h in svh.items() for d in (0, 2)}
    R.assert_cloud_edges(R.cloud_edges(host(xs), host(svh['splatting'].level(0).ijk), refs['splatting', 0].cnt), family)
    assert any((r.cnt == 0).any() for (kind, _), r in refs.items() if kind == 'neighbourhood')
    if family == 'A':
        assert all(r.on_plane > 0 for r in refs.values())
    return types.SimpleNamespace(ks=ks, xs=xs, ns=ns, svh=svh, refs=refs, n=xs.shape[0])


GRIDS = [(kind, d) for kind in ('splatting', 'neighbourhood') for d in (0, 2)]


def _features(family, n, C_):
    return R._values(np.random.default_rng([30, C_, int(family == 'A')]), (n, C_), family)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind,d', GRIDS)
def test_site_ranges(kind, d, family):
    from nksr_amd.nn.network import site_ranges
    c = _cloud(family)
    g = c.svh[kind].level(d)
    st, en = site_ranges(c.ks, g, d)
    want = R.site_ranges_ref(host(c.ks), host(g.keys), d)
    assert np.array_equal(host(st), want[0]) and np.array_equal(host(en), want[1])
    assert int((want[1] - want[0]).sum()) == c.n            # every point's cell is a voxel of either grid


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind,d', GRIDS)
def test_splat_trilinear(kind, d, family):
    from nksr_amd.nn.network import splat_trilinear
    c = _cloud(family)
    for C_ in (1, 3, 8):
        f = _features(family, c.n, C_)
        out, ws = splat_trilinear(c.svh[kind].level(d), d, R.INV_W0, c.ks, c.xs, dev(f))
        c.refs[kind, d].check_sum('splat_trilinear:%s:%s:L%d:C=%d' % (family, kind, d, C_), f, host(out), host(ws), pu.check)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind,d', GRIDS)
def test_splat_mean(kind, d, family):
    """C = 32: the half-wave kernel through the production wrapper; C = 5, 8, 20: the generic kernel (short last channel group)."""
    from nksr_amd.nn.network import splat_mean, site_ranges
    c = _cloud(family)
    g = c.svh[kind].level(d)
    for C_ in (32, 5, 8, 20):
        f = _features(family, c.n, C_)
        fd = dev(f)
        name = 'splat_mean:%s:%s:L%d:C=%d' % (family, kind, d, C_)
        if C_ == 32:
            out = splat_mean(g, d, R.INV_W0, c.ks, c.xs, fd)
        else:
            st, en = site_ranges(c.ks, g, d)
            buf, out = nan_padded(g.num_voxels, C_)
            call('nksr_splat_mean', ptr(c.xs), ptr(fd), C_, ptr(st), ptr(en), ptr(g.nbr), ptr(g.ijk), g.num_voxels,
                 float(R.INV_W0 * 2.0 ** (-d)), out.data_ptr(), stream())
            assert torch.isnan(buf[g.num_voxels:]).all(), name
        c.refs[kind, d].check_mean(name, f, host(out), pu.check)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind,d', GRIDS)
def test_splat_plane(kind, d, family):
    from nksr_amd.nn.network import splat_plane
    c = _cloud(family)
    out = splat_plane(c.svh[kind].level(d), d, R.INV_W0, c.ks, c.xs, c.ns)
    c.refs[kind, d].check_plane('splat_plane:%s:%s:L%d' % (family, kind, d), host(c.ns), host(out), pu.check)


@pytest.mark.parametrize('family', FAMILIES)
def test_splats_on_a_one_voxel_grid(family):
    """One voxel: one live half-wave whose partner and the six half-waves behind it are dead."""
    from nksr_amd.nn.network import sort_cloud, splat_trilinear, splat_mean, splat_plane
    from nksr_amd.svh import SparseFeatureHierarchy
    rng = np.random.default_rng(40)
    frac = rng.integers(0, 4, size=(9, 3)) / 4.0 + (0 if family == 'A' else rng.uniform(0.02, 0.23, size=(9, 3)))
    xyz = ((np.array([-2, 3, 1]) + frac) * R.VOXEL).astype(np.float32)
    ks, xs, ns = sort_cloud(dev(xyz), dev(R._values(rng, (9, 3), family, lim=2)), R.INV_W0)
    svh = SparseFeatureHierarchy(R.VOXEL, 1, 'cuda').build_from_grid_coords(0, torch.tensor([[-2, 3, 1]], dtype=torch.int32))
    g = svh.level(0)
    assert g.num_voxels == 1
    ref = R.SplatRef(host(xs), host(g.ijk), 0, family)
    assert ref.cnt[0] == 9
    name = 'one voxel:%s' % family
    f = _features(family, 9, 8)
    out, ws = splat_trilinear(g, 0, R.INV_W0, ks, xs, dev(f))
    ref.check_sum(name + ':trilinear', f, host(out), host(ws), pu.check)
    f = _features(family, 9, 32)
    ref.check_mean(name + ':mean32', f, host(splat_mean(g, 0, R.INV_W0, ks, xs, dev(f))), pu.check)
    f = _features(family, 9, 5)
    ref.check_mean(name + ':mean5', f, host(splat_mean(g, 0, R.INV_W0, ks, xs, dev(f))), pu.check)
    ref.check_plane(name + ':plane', host(ns), host(splat_plane(g, 0, R.INV_W0, ks, xs, ns)), pu.check)


def test_empty_cloud_onto_a_grid_with_voxels():
    """No point: zeros, decided in the wrappers (the kernels carry no point count and are not launched)."""
    from nksr_amd.nn.network import splat_trilinear, splat_mean, splat_plane
    g = _cloud('A').svh['splatting'].level(0)
    xs = torch.empty((0, 3), dtype=torch.float32, device='cuda')
    ks = torch.empty(0, dtype=torch.int64, device='cuda')
    out, ws = splat_trilinear(g, 0, R.INV_W0, ks, xs, torch.empty((0, 3), dtype=torch.float32, device='cuda'))
    assert out.shape == (g.num_voxels, 3) and ws.shape == (g.num_voxels,) and not out.any() and not ws.any()
    for C_ in (32, 5):
        m = splat_mean(g, 0, R.INV_W0, ks, xs, torch.empty((0, C_), dtype=torch.float32, device='cuda'))
        assert m.shape == (g.num_voxels, C_) and not m.any()
    p = splat_plane(g, 0, R.INV_W0, ks, xs, xs)
    assert p.shape == (g.num_voxels, 8) and not p.any()


@pytest.mark.parametrize('family', FAMILIES)
def test_point_encoder_forward(family):
    """PointEncoder._forward_hip = nksr_point_mlp, then splat_mean onto level 0: the MLP rows of the crafted cloud against the reference,
    the composition bit for bit against the two kernels called one after the other."""
    from nksr_amd.nn.network import PointEncoder, EncodedCloud, splat_mean
    c = _cloud(family)
    case = R.mlp_case(c.n, family)
    case['xyz'], case['feat'] = host(c.xs), host(c.ns)
    enc_mod = PointEncoder(types.SimpleNamespace(unet=types.SimpleNamespace(f_maps=32)))
    with torch.no_grad():
        for k in ('W1', 'b1', 'W2', 'b2'):
            getattr(enc_mod, k).copy_(torch.from_numpy(case[k]))
    enc_mod = enc_mod.cuda()
    enc = EncodedCloud()
    enc.keys, enc.xyz, enc.feat = c.ks, c.xs, c.ns
    svh = c.svh['splatting']
    vf = enc_mod._forward_hip(enc, svh, 0)
    buf, g = _mlp_direct(case, c.xs, c.ns)
    R.check_mlp('point_encoder:%s:mlp' % family, case, host(buf), pu.check)
    assert torch.equal(vf, splat_mean(svh.level(0), 0, R.INV_W0, c.ks, c.xs, g.contiguous()))
    if family == 'B':       # (the lattice rows are too large for an exact mean of 300 of them; the fp64 bound holds for any rows)
        c.refs['splatting', 0].check_mean('point_encoder:B:mean of the rows', host(g), host(vf), pu.check)


# ---- UDF decode -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _udf():
    from nksr_amd import _lib
    from nksr_amd.svh import SparseFeatureHierarchy
    case = R.udf_case()
    svh = SparseFeatureHierarchy(R.VOXEL, 1, 'cuda').build_from_grid_coords(0, torch.from_numpy(case['ijk']))
    g = svh.level(0)
    assert g.num_voxels == len(case['ijk'])
    row = host(g.ijk_to_index(dev(case['ijk']))).astype(np.int64)
    feat = np.zeros_like(case['feat'])
    feat[row] = case['feat']
    lv = _lib.LevelT()
    lv.n, lv.offset = g.num_voxels, 0
    lv.keys, lv.ijk, lv.nbr = ptr(g.keys), ptr(g.ijk), ptr(g.nbr)
    lv.hkeys, lv.hvals, lv.hcap = ptr(g.hash.hkeys), ptr(g.hash.hvals), g.hash.cap
    stats = {}
    fresh = R.udf_ref32(case['ijk'], case['feat'], case['xyz'], R.INV_W0, R.VOXEL, stats=stats)
    return types.SimpleNamespace(case=case, svh=svh, lv=lv, feat=dev(feat), xyz=dev(case['xyz']), fresh=fresh, stats=stats)


def _decode(u, lv, only_unset, out):
    call('nksr_udf_decode', C.byref(lv), 0, ptr(u.feat), ptr(u.xyz), u.xyz.shape[0], R.INV_W0, R.VOXEL, int(only_unset), ptr(out), stream())
    return host(out)


def test_udf_decode_one_level():
    from nksr_amd.nn.network import UDFDecoder
    u = _udf()
    s = u.stats
    assert min(s['all8'], s['some'], s['none'], s['unoccupied_corners'], s['absent_corners']) > 0, s
    nq = u.xyz.shape[0]
    got = _decode(u, u.lv, 0, torch.full((nq,), float('nan'), dtype=torch.float32, device='cuda'))
    R.check_udf('udf_decode', u.fresh, got)
    assert np.array_equal(host(UDFDecoder()(u.xyz, u.svh, [u.feat])), got)


def test_udf_decode_only_unset():
    u = _udf()
    prev = R.udf_prev(u.case, u.fresh)
    got = _decode(u, u.lv, 1, dev(prev))
    R.check_udf_only_unset('udf_decode:only_unset', u.case, prev, got)
    want = R.udf_ref32(u.case['ijk'], u.case['feat'], u.case['xyz'], R.INV_W0, R.VOXEL, only_unset=True, prev=prev)
    R.check_udf('udf_decode:only_unset:all', want, got)


def test_udf_decode_on_a_level_without_voxels():
    from nksr_amd import _lib
    u = _udf()
    prev = R.udf_prev(u.case, u.fresh)
    empty = _lib.LevelT()
    assert np.array_equal(_decode(u, empty, 1, dev(prev)), prev)
    assert (_decode(u, empty, 0, dev(prev)) == R.FAR).all()
