"""The lattice mesher's two short cuts (nksr_amd/meshing.py _extract) against the sequence they replace:
(1) the premise -- a point's field value does not depend on its batch mates; (2) the constrain-first pass against a numpy
restatement of the rule of k_mise_constrain and against evaluate-all + nksr_mise_constrain; (3) edge ids from a scan against
nksr_mc_emit + unique + look-up; (4) the whole extraction against the previous sequence restated from the retained entry points.
Everything is compared bit for bit."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _no_grad():           # (as under BaseField.extract_dual_mesh: _extract is called directly here)
    with torch.no_grad():
        yield


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


# ---- fields ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere_field():
    import nksr_amd
    from nksr_amd import configs, utils
    xyz, nrm = utils.synth_sphere(5000, 0.45, 0.003, seed=0)
    rec = nksr_amd.Reconstructor(_dev(), hparams=configs.get_hparams('ks', tree_depth=3))
    return rec.reconstruct(torch.from_numpy(xyz).to(_dev()), torch.from_numpy(nrm).to(_dev()), voxel_size=0.06, solver_tol=1e-6)


@functools.lru_cache(maxsize=None)
def _chunk_field():
    import nksr_amd
    from nksr_amd import configs, utils
    xyz, nrm = utils.synth_sphere(5000, 1.2, 0.005, seed=0)               # (chunk_size goes with the model's own voxel, 0.1)
    xyz = (xyz - xyz.min(0)).astype(np.float32)          # chunk grid origin = bbox min: the sphere straddles the seam at x = ext / 2
    ext = float(xyz[:, 0].max())
    rec = nksr_amd.Reconstructor(_dev(), hparams=configs.get_hparams('ks', tree_depth=3))
    fld = rec.reconstruct(torch.from_numpy(xyz).to(_dev()), torch.from_numpy(nrm).to(_dev()), detail_level=None, solver_tol=1e-6,
                          chunk_size=ext / 2 + 1e-3)
    assert fld.grid[0] == 2 and len(fld.fields) >= 2
    return fld


class _Analytic:
    """A closed-form field on the support of a solved one: what _extract reads of a field, nothing else."""
    scale, texture_field = 1.0, None

    def __init__(self, base, fn):
        self.svh, self.fn = base.svh, fn
        if hasattr(base, 'meshing_depth'):
            self.meshing_depth = base.meshing_depth

    def _evaluate_f_model(self, xyz, grad, max_points=1 << 22):
        from nksr_amd.fields.base_field import EvaluationResult
        return EvaluationResult(self.fn(xyz), None)

    def mask_vertices(self, xyz):
        return None


def _field(name):
    if name == 'sphere':
        return _sphere_field()
    if name == 'chunks':
        return _chunk_field()
    scale = 0.1 / 0.06                                   # model units: voxel 0.1, the sphere's radius 0.75
    if name == 'shell':         # two sheets at radius R -+ half a voxel: one base cell apart
        return _Analytic(_sphere_field(), lambda p: (p.norm(dim=1) - 0.45 * scale) ** 2 - 0.05 ** 2)
    return _Analytic(_sphere_field(), lambda p: p[:, 0] * 0 + 1)      # 'flat': no sign change


# ---- the previous sequence, from the retained entry points -----------------------------------------------------------------------------
def _base_cells(field, U):
    """The cell keys _extract starts from (one process: no ownership masks)."""
    from nksr_amd import ops
    from nksr_amd._lib import call, ptr, stream
    svh, dev = field.svh, field.svh.device
    adaptive = max(1, min(int(getattr(field, 'meshing_depth', 1)), svh.depth))
    raw = torch.empty(0, dtype=torch.int64, device=dev)
    for d in range(adaptive):
        g = svh.level(d)
        if g.num_voxels == 0:
            continue
        fl = torch.empty(g.num_voxels, dtype=torch.int32, device=dev)
        call('nksr_base_cell_flags', ptr(g.nbr), g.num_voxels, ptr(fl), stream())
        sel = ops.compact(fl)
        if sel.numel() == 0:
            continue
        S = U << d
        rd = torch.empty(sel.numel() * S ** 3, dtype=torch.int64, device=dev)
        if d == 0:
            call('nksr_base_cell_keys', ptr(g.ijk), ptr(sel), sel.numel(), U, ptr(rd), stream())
        else:
            call('nksr_level_cell_keys', ptr(g.ijk), ptr(sel), sel.numel(), d, U, ptr(rd), stream())
        raw = torch.cat([raw, rd])
    return raw


def _previous(field, mise_iter, U, max_points=1 << 22, trim=True):
    """evaluate all, nksr_mise_constrain, nksr_mc_emit, sort-unique, hash, nksr_mc_vertices; returns the mesh (v, f, edge_vkey,
    edge_axis -- None when empty) and what the levels went through (for the tests of the parts)."""
    from nksr_amd import meshing, ops
    from nksr_amd._lib import call, ptr, stream
    dev = field.svh.device
    w0 = field.svh.voxel_size
    raw = _base_cells(field, U)
    log = {'levels': []}
    if raw.numel() == 0:
        return None, log
    h, prev = w0 / U, None
    for m in range(mise_iter + 1):
        cells, vkeys, cidx, vhash = meshing._cell_vertices(raw)
        nv, nc = vkeys.numel(), cells.numel()
        pos = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        call('nksr_lattice_positions', ptr(vkeys), nv, float(h), float(0.5 * w0), ptr(pos), stream())
        f = field._evaluate_f_model(pos, False, max_points=max_points).value.contiguous()
        f_eval = f.clone()
        if prev is not None:
            ch, ah = prev[0], prev[2]
            call('nksr_mise_constrain', ptr(vkeys), nv, ptr(f), ptr(ch.hkeys), ptr(ch.hvals), ch.cap, ptr(prev[1]), ptr(ah.hkeys), ptr(ah.hvals),
                 ah.cap, stream())
        log['levels'].append(dict(vkeys=vkeys, cells=cells, cidx=cidx, pos=pos, f=f, f_eval=f_eval, prev=prev, h=h))
        config = torch.empty(nc, dtype=torch.int32, device=dev)
        ntri = torch.empty(nc + 1, dtype=torch.int32, device=dev)
        ntri[nc] = 0
        call('nksr_cell_config', ptr(cidx), ptr(f), nc, ptr(config), ptr(ntri), stream())
        if m < mise_iter:
            act = torch.empty(nc, dtype=torch.int32, device=dev)
            call('nksr_cell_active_flags', ptr(config), nc, ptr(act), stream())
            asel = ops.compact(act)
            if asel.numel() == 0:
                return None, log
            raw = torch.empty(asel.numel() * 8, dtype=torch.int64, device=dev)
            call('nksr_cell_children', ptr(cells), ptr(asel), asel.numel(), ptr(raw), stream())
            active = cells[asel.long()].contiguous()
            prev = (vhash, f, ops.HashTable(active), active)
            h = h / 2
    tri_off = ops.exclusive_sum_i32(ntri)
    T = int(tri_off[nc].item())
    log.update(config=config, tri_off=tri_off, T=T)
    if T == 0:
        return None, log
    ekeys = torch.empty(T * 3, dtype=torch.int64, device=dev)
    call('nksr_mc_emit', ptr(cidx), ptr(config), ptr(tri_off), nc, ptr(ekeys), stream())
    uek = ops.sort_unique(ekeys)
    faces = ops.HashTable(uek).query(ekeys).view(T, 3)
    ne = uek.numel()
    verts = torch.empty((ne, 3), dtype=torch.float32, device=dev)
    call('nksr_mc_vertices', ptr(uek), ne, ptr(vkeys), ptr(vhash.hkeys), ptr(vhash.hvals), vhash.cap, ptr(pos), ptr(f), float(h), ptr(verts), stream())
    ev = torch.div(uek, 3, rounding_mode='floor')
    edge_vkey, edge_axis = vkeys[ev], (uek - ev * 3).to(torch.int8)
    log.update(ekeys=ekeys, uek=uek, faces=faces)
    if trim:
        verts, faces, (edge_vkey, edge_axis) = meshing._trim(field, verts, faces, (edge_vkey, edge_axis), masked=True)
    res = meshing._result(field, verts, faces)
    return (res.v, res.f, edge_vkey, edge_axis), log


# ---- 1. the premise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sphere', 'chunks'])
def test_evaluation_does_not_depend_on_batch_mates(name):
    field = _field(name)
    _, log = _previous(field, 0, 1)
    pos = log['levels'][0]['pos']
    n = pos.shape[0]
    assert n > 2000
    f_all = log['levels'][0]['f']
    ev = lambda p, mp=1 << 22: field._evaluate_f_model(p.contiguous(), False, max_points=mp).value
    assert _same(ev(pos[::3]), f_all[::3].contiguous()), 'every third point'
    assert _same(ev(pos.flip(0)).flip(0).contiguous(), f_all), 'reversed order'
    assert _same(ev(pos, 1000), f_all), 'max_points = 1000'


# ---- 2. constrain first -----------------------------------------------------------------------------------------------------------------
def _encode(ijk):
    from nksr_amd._lib import call, ptr, stream
    c = torch.as_tensor(np.asarray(ijk, dtype=np.int32).reshape(-1, 3), device=_dev()).contiguous()
    k = torch.empty(c.shape[0], dtype=torch.int64, device=_dev())
    call('nksr_encode_keys', ptr(c), c.shape[0], -1, ptr(k), stream())
    return k


def _decode(keys):
    from nksr_amd._lib import call, ptr, stream
    g = torch.empty((keys.numel(), 3), dtype=torch.int32, device=keys.device)
    call('nksr_decode_keys', ptr(keys.contiguous()), keys.numel(), -1, ptr(g), stream())
    return g.cpu().numpy().astype(np.int64)


def _rule(g, cvert, fc, active):
    """The rule in the comment of k_mise_constrain for refined lattice coordinates g [n, 3]: cvert {coarse vertex: index into fc},
    active = set of refined coarse cells.  flag [n] = 1 where the evaluated value stays; val [n] fp32 = the replacement elsewhere
    (sums in fp32, in the order x, y, z)."""
    flag, val = np.ones(len(g), np.int32), np.zeros(len(g), np.float32)
    for i, c in enumerate(g.tolist()):
        odd = [v & 1 for v in c]
        k = sum(odd)
        if k == 3:
            continue
        if k == 0:
            j = cvert.get((c[0] >> 1, c[1] >> 1, c[2] >> 1))
            if j is not None:
                flag[i], val[i] = 0, fc[j]
            continue
        cell = [[(c[a] - 1) >> 1] if odd[a] else [(c[a] >> 1) - 1, c[a] >> 1] for a in range(3)]
        if all(q in active for q in itertools.product(*cell)):
            continue
        ends = [[(c[a] - 1) >> 1, ((c[a] - 1) >> 1) + 1] if odd[a] else [c[a] >> 1] for a in range(3)]
        js = [cvert.get(q) for q in itertools.product(*ends)]            # (product runs z fastest: the order x, y, z of the loops)
        if all(j is not None for j in js):
            s = np.float32(0)
            for j in js:
                s = np.float32(s + fc[j])
            flag[i], val[i] = 0, np.float32(s * np.float32(0.5 if k == 1 else 0.25))
    return flag, val


def _constrain_both(vkeys, ch, fc, ah, f_eval):
    """(flag, f) of the constrain-first pass on a poisoned f, and f_eval after nksr_mise_constrain"""
    from nksr_amd._lib import call, ptr, stream
    nv = vkeys.numel()
    f_new = torch.full((nv,), float('nan'), dtype=torch.float32, device=vkeys.device)
    flag = torch.full((nv,), -7, dtype=torch.int32, device=vkeys.device)
    call('nksr_mise_constrain_first', ptr(vkeys), nv, ptr(f_new), ptr(ch.hkeys), ptr(ch.hvals), ch.cap, ptr(fc), ptr(ah.hkeys), ptr(ah.hvals), ah.cap,
         ptr(flag), stream())
    f_old = f_eval.clone()
    call('nksr_mise_constrain', ptr(vkeys), nv, ptr(f_old), ptr(ch.hkeys), ptr(ch.hvals), ch.cap, ptr(fc), ptr(ah.hkeys), ptr(ah.hvals), ah.cap, stream())
    return flag, f_new, f_old


def _active_sets():
    rng = np.random.RandomState(7)
    blob = np.unique(rng.randint(-8, 8, size=(2600, 3)), axis=0)[:2000]          # across the origin: negative coordinates under the bias
    return {'one cell': [(0, 0, 0)],
            'slab 2x2x1': [(x, y, 0) for x in range(2) for y in range(2)],
            'block 2x2x2': list(itertools.product(range(2), repeat=3)),
            'L of three': [(0, 0, 0), (1, 0, 0), (0, 1, 0)],
            'sharing an edge': [(0, 0, 0), (1, 1, 0)],
            'sharing a corner': [(-1, -1, -1), (0, 0, 0)],
            'random 16^3': [tuple(r) for r in blob.tolist()]}


@pytest.mark.parametrize('name', list(_active_sets()))
def test_constrain_first_equals_the_rule(name):
    from nksr_amd import meshing, ops
    from nksr_amd._lib import call, ptr, stream
    rng = np.random.RandomState(11)
    active = ops.sort_unique(_encode(_active_sets()[name]))
    na = active.numel()
    _, cvk, _, _ = meshing._cell_vertices(active)                           # the coarse lattice: the corners of the active cells
    if name.startswith('random'):                                            # ... some of them missing: the rule then keeps the evaluated value
        cvk = cvk[torch.from_numpy(rng.rand(cvk.numel()) > 0.02).to(_dev())].contiguous()
    fc = torch.from_numpy(rng.standard_normal(cvk.numel()).astype(np.float32)).to(_dev())
    ch, ah = ops.HashTable(cvk), ops.HashTable(active)
    kids = torch.empty(na * 8, dtype=torch.int64, device=_dev())
    call('nksr_cell_children', ptr(active), ptr(torch.arange(na, dtype=torch.int32, device=_dev())), na, ptr(kids), stream())
    _, vkeys, _, _ = meshing._cell_vertices(kids)
    f_eval = torch.from_numpy(rng.standard_normal(vkeys.numel()).astype(np.float32)).to(_dev())
    flag, f_new, f_old = _constrain_both(vkeys, ch, fc, ah, f_eval)

    cvert = {tuple(c): j for j, c in enumerate(_decode(cvk).tolist())}
    rflag, rval = _rule(_decode(vkeys), cvert, fc.cpu().numpy(), set(map(tuple, _decode(active).tolist())))
    flag, f_new, f_old = flag.cpu().numpy(), f_new.cpu().numpy(), f_old.cpu().numpy()
    assert np.array_equal(flag, rflag)
    over = rflag == 0
    assert over.any() and (name != 'block 2x2x2' or int(rflag.sum()) == 8 + 6 + 12)      # the centres, the interior edges' and faces' midpoints stay
    assert np.array_equal(f_new[over].view(np.int32), rval[over].view(np.int32))
    assert np.array_equal(f_new[over].view(np.int32), f_old[over].view(np.int32))
    assert np.isnan(f_new[~over]).all(), 'the pass writes only what the rule replaces'
    assert np.array_equal(f_old[~over].view(np.int32), f_eval.cpu().numpy()[~over].view(np.int32))


def test_constrain_first_on_a_sphere():
    _, log = _previous(_sphere_field(), 1, 1)
    lv = log['levels'][1]
    vhash, fc, ah, active = lv['prev']
    flag, f_new, f_old = _constrain_both(lv['vkeys'], vhash, fc, ah, lv['f_eval'])
    cvert = {tuple(c): j for j, c in enumerate(_decode(log['levels'][0]['vkeys']).tolist())}
    rflag, rval = _rule(_decode(lv['vkeys']), cvert, fc.cpu().numpy(), set(map(tuple, _decode(active).tolist())))
    n, kept = len(rflag), int(rflag.sum())
    print('sphere, MISE level 1: %d of %d refined vertices are evaluated, %.1f %% are overwritten' % (kept, n, 100.0 * (n - kept) / n))
    assert int(flag.sum().item()) == kept and np.array_equal(flag.cpu().numpy(), rflag)
    over = rflag == 0
    assert np.array_equal(f_new.cpu().numpy()[over].view(np.int32), rval[over].view(np.int32))
    assert _same(torch.where(torch.from_numpy(over).to(_dev()), f_new, lv['f_eval']), f_old) and _same(f_old, lv['f'])


# ---- 3. edge ids ------------------------------------------------------------------------------------------------------------------------
def _edge_ids(cidx, config, tri_off, T, nv):
    from nksr_amd import ops
    from nksr_amd._lib import call, ptr, stream
    dev, nc = cidx.device, config.numel()
    used = torch.zeros(3 * nv + 1, dtype=torch.int32, device=dev)
    far = torch.full((3 * nv,), -5, dtype=torch.int32, device=dev)
    call('nksr_mc_mark_edges', ptr(cidx), ptr(config), nc, ptr(used), ptr(far), stream())
    eid = ops.exclusive_sum_i32(used)
    faces = torch.full((T, 3), -5, dtype=torch.int32, device=dev)
    call('nksr_mc_faces', ptr(cidx), ptr(config), ptr(tri_off), nc, ptr(eid), ptr(faces), stream())
    return used.cpu().numpy(), far.cpu().numpy(), eid.cpu().numpy(), faces.cpu().numpy()


def _check_edge_ids(cidx, config, tri_off, T, nv):
    from nksr_amd import ops
    from nksr_amd._lib import call, ptr, stream
    ekeys = torch.empty(T * 3, dtype=torch.int64, device=cidx.device)
    call('nksr_mc_emit', ptr(cidx), ptr(config), ptr(tri_off), config.numel(), ptr(ekeys), stream())
    uek = ops.sort_unique(ekeys)
    ref_faces = ops.HashTable(uek).query(ekeys).view(T, 3).cpu().numpy()
    keys = np.unique(ekeys.cpu().numpy())
    assert np.array_equal(keys, uek.cpu().numpy())
    used, far, eid, faces = _edge_ids(cidx, config, tri_off, T, nv)
    assert set(np.unique(used).tolist()) <= {0, 1} and used[3 * nv] == 0
    assert np.array_equal(np.flatnonzero(used), keys), 'the used slots are the unique keys'
    assert np.array_equal(eid[keys], np.arange(len(keys))) and eid[3 * nv] == len(keys)
    assert faces.dtype == ref_faces.dtype and np.array_equal(faces, ref_faces)
    # the far end: the corner one step along the axis from the lower end, in the cell that names the edge
    c = cidx.cpu().numpy()
    pair = {}
    for lo in range(8):
        for axis in range(3):
            if not lo & (4 >> axis):
                for a, b in zip(c[:, lo].tolist(), c[:, lo | (4 >> axis)].tolist()):
                    pair[3 * a + axis] = b
    assert np.array_equal(far[keys], np.array([pair[int(k)] for k in keys]))
    assert (far[used[:3 * nv] == 0] == -5).all(), 'an unused slot is not written'
    return len(keys)


def _configure(cidx, f):
    from nksr_amd import ops
    from nksr_amd._lib import call, ptr, stream
    nc = cidx.shape[0]
    config = torch.empty(nc, dtype=torch.int32, device=cidx.device)
    ntri = torch.zeros(nc + 1, dtype=torch.int32, device=cidx.device)
    call('nksr_cell_config', ptr(cidx), ptr(f), nc, ptr(config), ptr(ntri), stream())
    tri_off = ops.exclusive_sum_i32(ntri)
    return config, ntri, tri_off, int(tri_off[nc].item())


def test_edge_ids_on_a_sphere():
    _, log = _previous(_sphere_field(), 1, 3)            # (grid_upsample 3: nine times the edges of the plain lattice)
    lv = log['levels'][1]
    ne = _check_edge_ids(lv['cidx'], log['config'], log['tri_off'], log['T'], lv['vkeys'].numel())
    assert ne > 20000                                    # many scan tiles


def test_edge_ids_every_configuration():
    """256 separate cells, one per sign pattern: the five-triangle configurations are among them"""
    cidx = torch.arange(256 * 8, dtype=torch.int32, device=_dev()).view(256, 8).contiguous()
    sign = ((torch.arange(256, device=_dev())[:, None] >> torch.arange(8, device=_dev())[None]) & 1).to(torch.float32) * 2 - 1
    config, ntri, tri_off, T = _configure(cidx, sign.reshape(-1).contiguous())
    assert config.cpu().tolist() == list(range(256)) and int(ntri.max()) == 5
    _check_edge_ids(cidx, config, tri_off, T, 256 * 8)


def test_edge_ids_two_cells_sharing_one_cut_edge():
    """cells (0,0,0) and (1,1,0) meet in the lattice edge (1,1,0)-(1,1,1): corners 6, 7 of the first, 0, 1 of the second"""
    cidx = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7], [6, 7, 8, 9, 10, 11, 12, 13]], dtype=torch.int32, device=_dev())
    f = -torch.ones(14, dtype=torch.float32, device=_dev())
    f[6] = 1.0                                           # one positive vertex: its three edges are cut in both cells
    config, ntri, tri_off, T = _configure(cidx, f)
    assert ntri.cpu().tolist() == [1, 1, 0]
    assert _check_edge_ids(cidx, config, tri_off, T, 14) == 5            # 3 + 3 cut edges, the shared one (slot 3 * 6 + 2) once
    used, far, eid, faces = _edge_ids(cidx, config, tri_off, T, 14)
    assert used[3 * 6 + 2] == 1 and far[3 * 6 + 2] == 7
    assert len(set(faces[0].tolist()) & set(faces[1].tolist())) == 1


# ---- 4. the whole extraction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('upsample', [1, 2])
@pytest.mark.parametrize('mise_iter', [0, 1, 2])
@pytest.mark.parametrize('name', ['sphere', 'shell', 'flat', 'chunks'])
def test_extraction_equals_the_previous_sequence(name, mise_iter, upsample):
    from nksr_amd import meshing
    field = _field(name)
    ref, _ = _previous(field, mise_iter, upsample)
    res = meshing._extract(field, mise_iter, upsample, -1)
    if name == 'flat':
        assert ref is None
    else:
        assert ref is not None and ref[0].shape[0] > 100
    if ref is None:
        assert res.v.shape == (0, 3) and res.f.shape == (0, 3) and res.edge_vkey.numel() == 0 and res.edge_axis.numel() == 0
        return
    v, f, key, axis = ref
    assert _same(res.v, v), 'vertices'
    assert _same(res.f, f), 'faces'
    assert _same(res.edge_vkey, key) and _same(res.edge_axis, axis), 'vertex names'
    if name == 'shell' and mise_iter == 0 and upsample == 1:             # two sheets: two closed components' worth of vertices
        r = res.v.norm(dim=1)
        mid = 0.45 * 0.1 / 0.06
        assert int((r < mid).sum()) > 100 and int((r > mid).sum()) > 100
