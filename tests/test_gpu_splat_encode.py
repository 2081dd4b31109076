"""The encoder's one pass over the points (csrc/splat.hip: k_splat_encode32) against the two kernels it stands for, and
the U-Net's normal target taken from it by index against the splat on the candidate grid that it replaces.  Every comparison is bit
for bit (torch.equal on int32 views: +0.0 and -0.0 differ).

One crafted cloud of about 5 000 points serves all tests: a torus shell around the origin (negative coordinates), a thin double sheet
with opposed normals inside one layer of voxels, points exactly on voxel faces and half-faces (k w / 2) and one ulp to either side,
and isolated cells that hold 1, 4, 5, 9 and 40 points (the end of a round, two rounds, many rounds, a list of more than 16
entries) next to cells that hold none."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOXEL = 0.1
CELL_COUNTS = (1, 4, 5, 9, 40)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _crafted_cloud():
    from nksr_amd import utils
    rng = np.random.default_rng(7)
    w = np.float32(VOXEL)
    parts, normals = [], []
    xyz, nrm = utils.synth_torus(3500, 0.8, 0.3, 0.0, 1)
    parts.append(xyz.astype(np.float32)), normals.append(nrm.astype(np.float32))
    # a thin double sheet: both sides inside one layer of voxels, normals opposed
    m = 400
    xy = rng.uniform([1.5, -0.5], [2.5, 0.5], size=(2 * m, 2))
    z = np.where(np.arange(2 * m) < m, 0.021, 0.034)
    parts.append(np.column_stack([xy, z]).astype(np.float32))
    normals.append(np.column_stack([np.zeros((2 * m, 2)), np.where(np.arange(2 * m) < m, -1.0, 1.0)]).astype(np.float32))
    # faces and half-faces, and one ulp to either side of them
    k = np.arange(-7, 8, dtype=np.float32)
    on = (k * w / np.float32(2.0)).astype(np.float32)
    vals = np.concatenate([on, np.nextafter(on, np.float32(np.inf)), np.nextafter(on, np.float32(-np.inf))])
    face = vals[rng.integers(0, vals.size, size=(600, 3))] + np.array([-2.0, 1.5, -1.0], dtype=np.float32)
    parts.append(face.astype(np.float32))
    n = rng.normal(size=(600, 3))
    normals.append((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
    # isolated cells with a given number of points (five voxels apart: the cells between them hold none)
    for i, cnt in enumerate(CELL_COUNTS):
        cell = np.array([40 + 5 * i, -3, 2], dtype=np.float64)
        parts.append(((cell + rng.uniform(0.05, 0.95, size=(cnt, 3))) * VOXEL).astype(np.float32))
        n = rng.normal(size=(cnt, 3))
        normals.append((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
    return np.concatenate(parts), np.concatenate(normals)


@functools.lru_cache(None)
def _cloud():
    """The sorted cloud, both hierarchies over it (depth 4), 32 random feature channels per point and the two old splats of level 0."""
    from nksr_amd.nn.network import sort_cloud, splat_mean, splat_trilinear
    from nksr_amd.svh import SparseFeatureHierarchy, inv_w0_f32
    xyz, nrm = _crafted_cloud()
    c = types.SimpleNamespace()
    c.inv_w0 = inv_w0_f32(VOXEL)
    c.ks, c.xs, c.ns = sort_cloud(torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda(), c.inv_w0)
    c.cells = SparseFeatureHierarchy.cells_with_points(c.ks, 4)
    c.enc = SparseFeatureHierarchy(VOXEL, 4, 'cuda').build_point_splatting_sorted(c.xs, c.ks, c.cells)
    c.cand = SparseFeatureHierarchy(VOXEL, 4, 'cuda').build_point_neighborhood_sorted(c.ks, c.cells)
    c.f32 = torch.from_numpy(np.random.default_rng(8).normal(size=(c.xs.shape[0], 32)).astype(np.float32)).cuda()
    g = c.enc.level(0)
    c.mean_enc = splat_mean(g, 0, c.inv_w0, c.ks, c.xs, c.f32)
    c.sum_enc, c.ws_enc = splat_trilinear(g, 0, c.inv_w0, c.ks, c.xs, c.ns)
    return c


def test_cloud_is_what_the_tests_need():
    c = _cloud()
    assert 4500 <= c.xs.shape[0] <= 5500 and bool((c.xs < 0).any())
    cells0 = c.cells[0]
    cnt = torch.searchsorted(c.ks, cells0, right=True) - torch.searchsorted(c.ks, cells0)
    for want in CELL_COUNTS:
        assert bool((cnt == want).any()), 'no cell with %d points' % want
    assert int(cnt.max()) >= 40
    # voxels of the encoder grid whose own cell holds no point (their lane 13 lists nothing)
    assert c.enc.level(0).num_voxels > cells0.numel()


def test_premise_on_the_old_kernels():
    """k_splat_trilinear on the candidate grid (27-neighbourhood of the cells that hold points) is +0.0 on every voxel the encoder grid
    lacks, and on every voxel it has equals k_splat_trilinear on the encoder grid at the mapped index."""
    from nksr_amd.nn.network import splat_trilinear
    c = _cloud()
    gc, ge = c.cand.level(0), c.enc.level(0)
    out, ws = splat_trilinear(gc, 0, c.inv_w0, c.ks, c.xs, c.ns)
    je = ge.hash.query(gc.keys).long()
    absent = je < 0
    assert int(absent.sum()) > 0 and int((~absent).sum()) > 0
    assert not bits(out[absent]).any() and not bits(ws[absent]).any(), 'a candidate voxel outside the encoder grid carries weight'
    assert same(out[~absent], c.sum_enc[je[~absent]]) and same(ws[~absent], c.ws_enc[je[~absent]])
    # every cell that holds a point is a voxel of the encoder grid (what keeps the neighbour rows of both grids alike)
    assert bool((ge.hash.query(c.cells[0]) >= 0).all())


def _grids():
    """Level 0 of the encoder hierarchy, the same without its last voxel (one of the two has an odd number of voxels: a dead half-wave
    next to a live one), and a grid of one voxel: the cell of 40 points."""
    from nksr_amd.svh import SparseFeatureHierarchy, SparseGrid
    c = _cloud()
    g = c.enc.level(0)
    one = SparseFeatureHierarchy(VOXEL, 1, 'cuda').build_from_grid_coords(0, torch.tensor([[40 + 5 * 4, -3, 2]], dtype=torch.int32)).level(0)
    assert one.num_voxels == 1
    return [('level 0', g), ('level 0 less one', SparseGrid(g.keys[:-1].contiguous(), 0, VOXEL)), ('one voxel', one)]


def test_splat_encode_equals_the_two_splats():
    from nksr_amd.nn.network import splat_encode, splat_mean, splat_trilinear
    c = _cloud()
    odd = 0
    for name, g in _grids():
        odd += g.num_voxels & 1
        mean = splat_mean(g, 0, c.inv_w0, c.ks, c.xs, c.f32)
        s, ws = splat_trilinear(g, 0, c.inv_w0, c.ks, c.xs, c.ns)
        assert bool(ws.any()), name
        vf, ns, w = splat_encode(g, 0, c.inv_w0, c.ks, c.xs, c.f32, c.ns)
        assert same(vf, mean), name + ': voxel_feat'
        assert same(ns, s), name + ': normal_sum'
        assert same(w, ws), name + ': weight_sum'
        vf, ns, w = splat_encode(g, 0, c.inv_w0, c.ks, c.xs, c.f32, None)
        assert same(vf, mean) and ns is None and w is None, name + ': without normals'
    assert odd >= 2           # (the one-voxel grid and one of the other two)
    assert same(splat_encode(c.enc.level(0), 0, c.inv_w0, c.ks, c.xs, c.f32, c.ns)[1], c.sum_enc)      # (two runs agree)


def test_null_normals_leave_their_outputs_alone():
    """The C entry with a NULL normals pointer: voxel_feat as ever, normal_sum / weight_sum not written (and allowed to be NULL)."""
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.nn.network import site_ranges
    c = _cloud()
    g = c.enc.level(0)
    n = g.num_voxels
    st, en = site_ranges(c.ks, g, 0)
    vf = torch.full((n, 32), float('nan'), device='cuda')
    ns = torch.full((n, 3), float('nan'), device='cuda')
    ws = torch.full((n,), float('nan'), device='cuda')
    call('nksr_splat_encode', ptr(c.xs), ptr(c.f32), None, ptr(st), ptr(en), ptr(g.nbr), ptr(g.ijk), n, float(c.inv_w0), ptr(vf), ptr(ns), ptr(ws), stream())
    assert same(vf, c.mean_enc) and bool(ns.isnan().all()) and bool(ws.isnan().all())
    vf.fill_(float('nan'))
    call('nksr_splat_encode', ptr(c.xs), ptr(c.f32), None, ptr(st), ptr(en), ptr(g.nbr), ptr(g.ijk), n, float(c.inv_w0), ptr(vf), None, None, stream())
    assert same(vf, c.mean_enc)
    call('nksr_splat_encode', ptr(c.xs), ptr(c.f32), ptr(c.ns), ptr(st), ptr(en), ptr(g.nbr), ptr(g.ijk), n, float(c.inv_w0), ptr(vf), ptr(ns), ptr(ws), stream())
    assert same(ns, c.sum_enc) and same(ws, c.ws_enc)


def test_splat_encode_of_an_empty_cloud():
    from nksr_amd.nn.network import splat_encode
    g = _cloud().enc.level(0)
    xs = torch.empty((0, 3), dtype=torch.float32, device='cuda')
    ks = torch.empty(0, dtype=torch.int64, device='cuda')
    vf, ns, ws = splat_encode(g, 0, _cloud().inv_w0, ks, xs, torch.empty((0, 32), dtype=torch.float32, device='cuda'), xs)
    assert vf.shape == (g.num_voxels, 32) and ns.shape == (g.num_voxels, 3) and ws.shape == (g.num_voxels,)
    assert not bits(vf).any() and not bits(ns).any() and not bits(ws).any()


# ---- the network ----------------------------------------------------------------------------------------------------------------------
def _network(preset, prune):
    from nksr_amd import configs
    from nksr_amd.nn.network import NKSRNetwork
    hp = configs.get_hparams(preset, voxel_size=VOXEL, head_init_scale=0.7, seed=3)
    net = NKSRNetwork(hp)
    rs = np.random.RandomState(0)
    for m in list(net.unet.down) + list(net.unet.up):
        m.bias.data = torch.from_numpy(rs.randn(32).astype(np.float32) * 0.1)
    if prune:       # the (random) structure head decides: decoder levels that are not the candidate levels
        for h in net.unet.structure_heads:
            h.bias.data.zero_()
            h.weight.data *= 4.0
    return hp, net.cuda().eval()


def _old_encoder(net, c):
    """What PointEncoder._forward_hip did: nksr_point_mlp, then splat_mean onto level 0; no splat of the normals is kept."""
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.nn.network import EncodedCloud, splat_mean
    e = net.encoder
    n = c.xs.shape[0]
    g = torch.empty((n, 32), dtype=torch.float32, device='cuda')
    call('nksr_point_mlp', ptr(c.xs), ptr(c.ns), n, c.enc.inv_w0, 32, ptr(e.W1.detach().contiguous()), ptr(e.b1.detach().contiguous()),
         ptr(e.W2.detach().contiguous()), ptr(e.b2.detach().contiguous()), ptr(g), stream())
    enc = EncodedCloud()
    enc.keys, enc.xyz, enc.feat, enc.cells = c.ks, c.xs, c.ns, c.cells
    enc.voxel_feat = splat_mean(c.enc.level(0), 0, c.enc.inv_w0, c.ks, c.xs, g)
    return enc


def _old_normals(net, hp, c, cand, dec, trunk, d):
    """feat.normal_features[d] as StructureUNet formed it: the splat on the candidate grid, the rows of the surviving voxels."""
    from nksr_amd.nn.network import splat_trilinear, gather_rows
    s, ws = splat_trilinear(cand.level(d), d, c.enc.inv_w0, c.ks, c.xs, c.ns)
    sel = cand.level(d).hash.query(dec.level(d).keys)      # (every row where no voxel was pruned: a copy)
    assert bool((sel >= 0).all())
    s, ws = gather_rows(s, sel), ws[sel.long()]
    nv = s + net.unet.normal_heads[d](trunk[d])
    nn_ = nv.norm(dim=1)
    den = torch.maximum(nn_, float(hp.normal_min_length) * ws).clamp_min(max(float(hp.normal_min_weight), 1e-30))
    return nv / den[:, None]


@pytest.mark.parametrize('case', ['adaptive 1', 'adaptive 1 pruned', 'adaptive 2', 'given structure', 'carla', 'carla pruned'])
def test_network_features_equal_the_old_call_sequence(case, monkeypatch):
    from nksr_amd.nn import network as N
    from nksr_amd.svh import SparseFeatureHierarchy
    c = _cloud()
    preset = 'carla' if case.startswith('carla') else 'ks'
    hp, net = _network(preset, case.endswith('pruned'))
    ad = {'adaptive 1': 1, 'adaptive 1 pruned': 1, 'adaptive 2': 2, 'given structure': 2, 'carla': int(hp.adaptive_depth), 'carla pruned': int(hp.adaptive_depth)}[case]
    assert preset != 'carla' or (ad == 2 and bool(hp.udf.enabled))
    gt = None
    if case == 'given structure':       # the neighbourhood of every third point: it lacks cells that hold points
        sub = c.ks[::3].contiguous()
        gt = SparseFeatureHierarchy(VOXEL, 4, 'cuda').build_point_neighborhood_sorted(sub)
        assert bool((gt.level(0).hash.query(c.cells[0]) < 0).any())
    with torch.no_grad():
        old_enc = _old_encoder(net, c)
        assert old_enc.normal_splat is None
        feat_o, dec_o, _ = net.unet._forward_impl(old_enc, c.enc, ad, gt, None)
        calls = []
        real = N.splat_trilinear
        monkeypatch.setattr(N, 'splat_trilinear', lambda grid, d, *a: (calls.append(d), real(grid, d, *a))[1])
        enc = net.encoder(c.xs, c.ns, c.enc, 0, sorted_keys=c.ks)
        enc.cells = c.cells
        assert enc.normal_splat is not None and same(enc.voxel_feat, old_enc.voxel_feat)
        assert same(enc.normal_splat[2], c.sum_enc) and same(enc.normal_splat[3], c.ws_enc)
        feat, dec, _ = net.unet._forward_impl(enc, c.enc, ad, gt, None)
        monkeypatch.undo()
        # the splat of level 0 is taken from the encoder's pass unless a structure is given; every other level splats as before
        assert calls == (list(range(ad)) if gt is not None else list(range(1, ad))), calls
        if case.endswith('pruned'):
            assert dec.level(0).num_voxels < c.cand.level(0).num_voxels
        for d in range(4):
            assert same(dec.level(d).keys, dec_o.level(d).keys), (case, d)
            assert same(feat.trunk_features[d], feat_o.trunk_features[d]), (case, d)
            assert same(feat.structure_features[d], feat_o.structure_features[d]), (case, d)
            assert same(feat.basis_features[d], feat_o.basis_features[d]), (case, d)
            assert (feat.normal_features[d] is None) == (d >= ad)
            if d < ad:
                assert same(feat.normal_features[d], feat_o.normal_features[d]), (case, d)
                assert same(feat.normal_features[d], _old_normals(net, hp, c, gt if gt is not None else c.cand, dec, feat.trunk_features, d)), (case, d)
                if bool(hp.udf.enabled):
                    assert same(feat.udf_features[d], feat_o.udf_features[d]), (case, d)

