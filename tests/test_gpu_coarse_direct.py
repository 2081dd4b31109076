"""The packed coarse-level block straight from the row fill (csrc/assemble.hip: k_row_diag, k_row_fill<.., true>; csrc/packed_rows.hip: k_pk_*; fields/assembly.py:
assemble_packed) against the path it replaces on the same field: fld.assemble(coarse_from=..., fused_op=op) -- the fp32 CSR -- followed
by _pack_block (nksr_coarse_pack_count / nksr_coarse_pack), which coarse_precond still takes with {'direct': False}.

Everything is compared word for word with nothing skipped: packed, packed_rowptr, dis, old_of_new, seg_base and the lambda / gershgorin
arrays; the early diagonal against the fill's.  There is no tolerance in this file: the new path forms the same fp32 sums in the same
order, rounds the same products to half precision and applies the same drop rule, so any difference is a mistake.

Fields: a noisy sphere of 36 voxels radius (4 000 points, ~1e5 finest voxels), tree depths 3, 4 and 5 with first_level 2 -- one, two and
three coarse levels, hence 0, 1 and 3 cross-level pairs -- alone, and as batches of two (depth 5) and three (depth 4) chunks: copies of
the cloud with their own noise, each inside its own aligned cube of 256 voxels, which is what a chunk of a batched solve is (Segments).
Every fixture is asserted to hold what its case is for."""
import numpy as np
import pytest
import torch

from conftest import make_cloud
import parity_util as pu

pytestmark = pytest.mark.gpu

C0 = 2
CUBE_BITS = 8                     # a chunk's cube: 2^8 finest voxels = 25.6 model units on a side
FIELDS = {'depth3': (3, 1), 'depth4': (4, 1), 'depth5': (5, 1), 'depth5x2': (5, 2), 'depth4x3': (4, 3)}
DROPS = [0.0, 0.005, 0.5]
_fields, _ops, _refs = {}, {}, {}


def _dev():
    return torch.device('cuda:0')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _field(name):
    """(svh, features, network, segments or None, position sites, normal sites, normal targets) of a fixture, built once"""
    if name not in _fields:
        from nksr_amd.fields.kernel_field import Segments
        depth, nchunk = FIELDS[name]
        side = 0.1 * (1 << CUBE_BITS)
        parts = []
        for c in range(nchunk):
            xyz, _ = make_cloud('sphere', 4000, 0.005, 11 + c)
            xyz = xyz * np.float32(8.0) + np.float32(0.5 * side)          # centred in the cube [0, side)^3 ...
            xyz[:, 0] += np.float32(c * side)                               # ... of chunk c
            parts.append(xyz.astype(np.float32))
        xyz = np.concatenate(parts)
        oh, svh, feats, _, net = pu.field_inputs(xyz, _dev(), depth=depth, seed=7)
        seg = None
        if nchunk > 1:
            cube = torch.unique(svh.level(0).keys >> (3 * CUBE_BITS))
            assert cube.numel() == nchunk, 'the chunks do not lie in %d cubes' % nchunk
            seg = Segments(svh, cube << (3 * CUBE_BITS), (cube + 1) << (3 * CUBE_BITS))
        nrm = oh.levels[0].centers().astype(np.float32)
        nval = np.random.RandomState(5).randn(len(nrm), 3).astype(np.float32)
        _fields[name] = (svh, feats, net, seg, xyz, nrm, nval)
    return _fields[name]


def _operator(name, row_format):
    """(KernelField, operator, segments) of a fixture in one row format, built once"""
    if (name, row_format) not in _ops:
        from nksr_amd.fields import KernelField
        svh, feats, net, seg, xyz, nrm, nval = _field(name)
        fld = KernelField(svh, net.interpolators, [torch.from_numpy(f) for f in feats])
        fld.solver_config['row_format'] = row_format
        op = fld.fused_operator(_t(xyz), _t(nrm), _t(nval), 1e4 / len(xyz), 1e2 / len(nrm), segments=seg)
        assert op['row_format'] == row_format
        _ops[(name, row_format)] = (fld, op, seg)
    return _ops[(name, row_format)]


def _reference(name, row_format, reg):
    """The fp32 CSR of the block (rowptr, cols, vals, diag as numpy) and the level of every coarse unknown, computed once"""
    key = (name, row_format, reg)
    if key not in _refs:
        fld, op, seg = _operator(name, row_format)
        rp, cc, vv, dd, _ = fld.assemble(None, None, None, 1.0, 1.0, reg, coarse_from=C0, fused_op=op)
        off = fld.svh.offsets
        n = fld.svh.num_unknowns - off[C0]
        level = np.concatenate([np.full(fld.svh.level(d).num_voxels, d) for d in range(C0, fld.svh.depth)])
        assert len(level) == n
        _refs[key] = dict(rowptr=rp.cpu().numpy(), cols=cc.cpu().numpy(), vals=vv.cpu().numpy(), diag=dd, level=level, n=n)
    return _refs[key]


def _blocks(name, row_format, drop, reg):
    """coarse_precond of the fixture through the direct path and through the CSR + nksr_coarse_pack"""
    fld, op, seg = _operator(name, row_format)
    out = {}
    for direct in (True, False):
        fld.solver_config['coarse_precond'] = {'first_level': C0, 'drop': drop, 'direct': direct}
        out[direct] = fld._coarse_precond(op, reg, seg)
        assert out[direct]['packed'] and out[direct]['first_level'] == C0
    fld.solver_config.pop('coarse_precond')
    return out[True], out[False]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _compare(new, ref):
    for k in ('unknowns', 'nnz', 'nnz_kept', 'steps', 'drop'):
        assert new[k] == ref[k], (k, new[k], ref[k])
    kept = new['nnz_kept'] - new['unknowns']
    names = ('packed', 'packed_rowptr', 'dis', 'old_of_new', 'seg_base', 'row_seg')
    for k, a, b in zip(names, new['keep'][:6], ref['keep'][:6]):
        if k == 'packed':
            a, b = a[:kept], b[:kept]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(_bits(a), _bits(b)), '%s differs in %d of %d words' % (k, int((_bits(a) != _bits(b)).sum()), a.numel())
    for k in ('lambda', 'gershgorin'):
        assert torch.equal(_bits(new[k]), _bits(ref[k])), (k, new[k], ref[k])
    return kept


def _fixture_properties(name, row_format, drop, ref, blk):
    """What the case is there for, from the reference CSR and the reference's packed rows"""
    fld, op, seg = _operator(name, row_format)
    n, level, rowptr, cols = ref['n'], ref['level'], ref['rowptr'], ref['cols']
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    offd = cols != rows
    assert int((~offd).sum()) == n                                       # one diagonal entry per row
    if seg is not None:      # chunks: no entry couples two segments (16-bit columns are local to the row's segment)
        rs = seg.unknown_seg[fld.svh.offsets[C0]:].cpu().numpy()
        assert np.array_equal(rs[rows], rs[cols]) and len(np.unique(rs)) == FIELDS[name][1]
    packed, prow, _, o2n, seg_base, row_seg_new = (a.cpu().numpy() for a in blk['keep'][:6])
    kept = blk['nnz_kept'] - n
    lens = np.diff(prow)
    prow_new = np.repeat(np.arange(n), lens)
    pcol_new = (packed[:kept].view(np.uint32) & 0xFFFF).astype(np.int64) + seg_base[row_seg_new[prow_new]]
    prow_old, pcol_old = o2n[prow_new], o2n[pcol_new]
    pairs = [(a, b) for a in range(C0, fld.svh.depth) for b in range(a + 1, fld.svh.depth)]
    assert len(pairs) == {3: 0, 4: 1, 5: 3}[fld.svh.depth]
    # mirrors: entries of a row whose column lies on a FINER level
    mir_struct = {p: int(((level[cols] == p[0]) & (level[rows] == p[1])).sum()) for p in pairs}
    mir_kept = {p: int(((level[pcol_old] == p[0]) & (level[prow_old] == p[1])).sum()) for p in pairs}
    pu.report('coarse_direct:%s:drop%g' % (name, drop), unknowns=n, structural=int(offd.sum()), kept=int(kept), rows_without_entry=int((lens == 0).sum()),
              mirrors=str(mir_struct), mirrors_kept=str(mir_kept))
    if drop == 0.0:
        assert kept == int(offd.sum()), 'drop 0 must keep every structural off-diagonal entry'
    if drop == 0.005:
        for p in pairs:
            assert 0 < mir_kept[p] < mir_struct[p], 'level pair %s: %d of %d mirrors kept' % (p, mir_kept[p], mir_struct[p])
    if drop == 0.5:
        assert (lens == 0).any(), 'no row is left without an entry'
        if pairs:            # rows whose mirrors all go: they have structural mirrors and keep none
            has = np.bincount(rows[level[cols] < level[rows]], minlength=n) > 0
            keeps = np.bincount(prow_old[level[pcol_old] < level[prow_old]], minlength=n) > 0
            assert (has & ~keeps).any()


@pytest.mark.parametrize('drop', DROPS, ids=['drop0', 'drop0.005', 'drop0.5'])
@pytest.mark.parametrize('row_format', ['dense', 'factors'])
@pytest.mark.parametrize('name', list(FIELDS))
def test_direct_block_equals_the_packed_csr_word_for_word(name, row_format, drop):
    new, ref = _blocks(name, row_format, drop, 1.0)
    _compare(new, ref)
    _fixture_properties(name, row_format, drop, _reference(name, row_format, 1.0), ref)


@pytest.mark.parametrize('name', ['depth5', 'depth5x2'])
def test_direct_block_with_another_regularisation_weight(name):
    """reg enters the diagonal alone: D^-1/2, every scaled value and with them the kept pattern move"""
    new, ref = _blocks(name, 'dense', 0.005, 0.25)
    _compare(new, ref)
    one = _blocks(name, 'dense', 0.005, 1.0)[0]
    assert not torch.equal(_bits(new['keep'][2]), _bits(one['keep'][2]))          # (dis did change)


@pytest.mark.parametrize('row_format', ['dense', 'factors'])
@pytest.mark.parametrize('name', list(FIELDS))
def test_early_diagonal_is_the_fills_bit_for_bit(name, row_format):
    """k_row_diag (ahead of the fill) against diag of the CSR fill, reg 1 and 0.25; and the parts of assemble_packed's result that
    coarse_precond does not pass on"""
    from nksr_amd.fields import assembly
    from nksr_amd.fields.coarse_precond import _renumber
    fld, op, seg = _operator(name, row_format)
    for reg in (1.0, 0.25):
        ref = _reference(name, row_format, reg)
        n = ref['n']
        rs = seg.unknown_seg[fld.svh.offsets[C0]:].contiguous() if seg is not None else torch.zeros(n, dtype=torch.int32, device=_dev())
        counts = torch.bincount(rs.long(), minlength=seg.nseg if seg is not None else 1)
        o2n, n2o, seg_base, _ = _renumber(n, rs, counts)
        local = (n2o - seg_base[rs.long()]).contiguous()
        assert int(local.min()) >= 0 and int(local.max()) < 65536
        packed, prow, dis, kept, nnz, diag = assembly.assemble_packed(fld, reg, C0, op, o2n, n2o, local, 0.005)
        assert torch.equal(diag.view(torch.int32), ref['diag'].view(torch.int32)), 'diagonal differs in %d of %d rows' % (int((diag != ref['diag']).sum()), n)
        assert nnz == len(ref['cols']) and kept == int(prow[n]) and float(diag.min()) > 0
        assert packed.numel() >= max(kept, 1) and dis.numel() == n


@pytest.mark.parametrize('row_format', ['dense', 'factors'])
@pytest.mark.parametrize('name', ['depth5', 'depth5x2'])
def test_level_aligned_gram_loads_give_the_site_set_blocks_bit_for_bit(name, row_format, monkeypatch):
    """The Gram kernels read the operator's row list with tile n = level d + n (asm_lm_pointers); handed over as a site set WITH a row
    index (the identity) the same rows go through gram_rows (csrc/gram.hip), whose loads and column map are the concatenated-levels ones.
    Both get the rows' targets as right-hand side, so the spare lane that carries it is compared too (b is not all zero).  Depth 5:
    three, two and one column tiles."""
    from nksr_amd._lib import ptr
    from nksr_amd.fields import assembly
    fld, op, seg = _operator(name, row_format)
    plain = assembly._sets_from_operator
    ident = torch.arange(op['rows_total'], dtype=torch.int32, device=_dev())

    def with_targets(indexed):
        def sets_from_operator(fld_, fused_op, coarse_from, sets, keep):
            nsets = plain(fld_, fused_op, coarse_from, sets, keep)
            sets[0].target = ptr(fused_op['targets_all'])
            if indexed:
                sets[0].row_index = ptr(ident)
            return nsets
        return sets_from_operator
    out = {}
    for indexed in (False, True):
        monkeypatch.setattr(assembly, '_sets_from_operator', with_targets(indexed))
        out[indexed] = fld.assemble(None, None, None, 1.0, 1.0, 1.0, coarse_from=C0, fused_op=op)
    for k, a, b in zip(('rowptr', 'cols', 'vals', 'diag', 'b'), out[False], out[True]):
        assert torch.equal(_bits(a), _bits(b)), '%s differs in %d of %d words' % (k, int((_bits(a) != _bits(b)).sum()), a.numel())
    assert float(out[False][4].abs().max()) > 0


def _level_parts(d):
    """asm_level_parts of csrc/gram.hip: the parts a level's cells are cut into at most"""
    return min(4 ** (d - 2), 64) if d >= 3 else 1


SPLIT_CASES = [('depth5', 'list'), ('depth5x2', 'list'), ('depth5x2', 'indexed'), ('depth4', 'sites')]


@pytest.mark.parametrize('name,source', SPLIT_CASES, ids=['%s-%s' % c for c in SPLIT_CASES])
def test_split_schedules_give_the_same_blocks_bit_for_bit(name, source, monkeypatch):
    """csrc/gram.hip cuts the rows of a cell of a level >= 3 into parts and promises the same block from both schedules of the parts:
    one wavefront per (cell, part) and a reduction through the split scratch (k_cell_blocks_part / _reduce: what every fixture of this
    size runs) and one wavefront per cell (k_cell_blocks_seq: what a level of more than 65536 (cell, part) pairs runs, the batched scene
    among them).  The same assembly with the scratch and without it, every returned tensor word for word.
    'list': the coarse block from the operator's row list (asm_accumulate_lm inside the split kernels); 'indexed': the same rows as a
    site set with the identity row index and their targets (gram_rows inside them, and a right-hand side); 'sites': the whole
    site-major system of the cloud, whose coarsest level splits."""
    from nksr_amd._lib import ptr
    from nksr_amd.fields import assembly
    fld, op, seg = _operator(name, 'dense')
    svh, _, _, _, xyz, nrm, nval = _field(name)
    off = fld.svh.offsets
    if source == 'sites':
        args = (_t(xyz), _t(nrm), _t(nval), 1e4 / len(xyz), 1e2 / len(nrm), 1.0)
        kwargs = {}
        rows = [0] * fld.svh.depth
        for ss in fld._site_sets((args[0], None, args[3], None), (args[1], args[2], args[4], None)):
            st, en = fld._site_ranges(ss.keys)
            rows = [r + (e - s).long() * ss.rows for r, s, e in zip(rows, st, en)]
    else:
        args, kwargs = (None, None, None, 1.0, 1.0, 1.0), dict(coarse_from=C0, fused_op=op)
        per_cell = (op['span'][1] - op['span'][0] + 1).long() * (op['span'][0] >= 0)
        rows = [per_cell[off[d]:off[d] + fld.svh.level(d).num_voxels] for d in range(fld.svh.depth)]
        if source == 'indexed':
            plain = assembly._sets_from_operator
            ident = torch.arange(op['rows_total'], dtype=torch.int32, device=_dev())

            def sets_from_operator(fld_, fused_op, coarse_from, sets, keep):
                nsets = plain(fld_, fused_op, coarse_from, sets, keep)
                sets[0].target, sets[0].row_index = ptr(fused_op['targets_all']), ptr(ident)
                return nsets
            monkeypatch.setattr(assembly, '_sets_from_operator', sets_from_operator)
    # the fixture holds its case: a level that splits has a cell of at least two parts, and few enough (cell, part) pairs for the
    # parallel schedule, whose scratch the first run is given
    split = [d for d in range(3, fld.svh.depth) if int(rows[d].max()) >= 256 and rows[d].numel() * _level_parts(d) <= 65536]
    assert split, [(d, int(rows[d].max()), rows[d].numel()) for d in range(fld.svh.depth)]
    given = []
    real = assembly._split_scratch

    def recorded(*a):
        given.append(real(*a))
        return given[-1]
    monkeypatch.setattr(assembly, '_split_scratch', recorded)
    par = fld.assemble(*args, **kwargs)
    assert len(given) == 1 and given[0][0] is not None and given[0][1] > 0
    monkeypatch.setattr(assembly, '_split_scratch', lambda *a: (None, 0))
    seq = fld.assemble(*args, **kwargs)
    pu.report('split_schedules:%s:%s' % (name, source), levels=str(split), largest_cell=str([int(rows[d].max()) for d in split]),
              cells=str([rows[d].numel() for d in split]), scratch_bytes=given[0][1])
    for k, a, b in zip(('rowptr', 'cols', 'vals', 'diag', 'b'), par, seq):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(_bits(a), _bits(b)), '%s differs in %d of %d words' % (k, int((_bits(a) != _bits(b)).sum()), a.numel())
    if source != 'list':
        assert float(par[4].abs().max()) > 0
