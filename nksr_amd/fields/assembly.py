"""CSR assembly of a KernelField's normal equations (csrc/gram.hip, assemble.hip, packed_rows.hip): the whole system of the assembled solve, or the
diagonal block of the coarse levels for the preconditioner -- from site sets or from the rows a matrix-free operator holds."""
import ctypes as C
import time

import torch

from .. import _lib, ops
from .._lib import SiteSetT, call, ptr, stream
from ._timing import _tick


def _sets_from_operator(fld, fused_op, coarse_from, sets, keep):
    """The operator's Morton-ordered row list IS a site set with one row per "site": the rows of a cell are the run
    span[0][j] .. span[1][j] (fused tables), so neither site ranges nor a row index are needed."""
    first, last = fused_op['span'][0], fused_op['span'][1]
    st_all, en_all = first.clamp(min=0), (last + 1).contiguous()
    off = fld.svh.offsets
    S = sets[0]
    S.n, S.ncomp, S.weight = fused_op['rows_total'], 1, 1.0
    if fused_op.get('row_format') == 'factors':
        # the factor form holds no dense rows: those of the levels >= coarse_from were written out by the set-up sweep
        # (or are expanded now); the array starts at level coarse_from (nksr_siteset_t.level_base)
        dense = fld._dense_coarse_rows(fused_op, int(coarse_from))
        S.val, S.level_base = ptr(dense), int(coarse_from)
        keep.append(dense)
    else:
        S.val = ptr(fused_op['rows_all'])
    S.level_stride = fused_op['rows_total']
    for d in range(fld.svh.depth):
        nd = fld.svh.level(d).num_voxels
        S.start[d], S.end[d] = ptr(st_all[off[d]:off[d] + nd]), ptr(en_all[off[d]:off[d] + nd])
    keep += [st_all, en_all]
    return 1


def _sets_from_sites(fld, site_sets, hier, sets, keep):
    """One nksr_siteset_t per prepared site set (KernelField._site_sets): its kernel rows in ``hier`` and its sites' run per cell.
    Rows (and targets) are produced pre-multiplied by sqrt(weight): the Gram products of the assembly are then bitwise
    symmetric and its matrix-core operands need no scaling."""
    for S, ss in zip(sets, site_sets):
        val, dval = fld.kernel_rows(ss.xs, grad=ss.grad, scale=ss.sw, values=not ss.grad, hier=hier)
        rows = dval if ss.grad else val
        st, en = fld._site_ranges(ss.keys)
        S.n, S.ncomp, S.weight = ss.xs.shape[0], ss.rows, 1.0
        S.val = ptr(rows)
        tgt = None
        if ss.target is not None:
            tgt = ss.target.to(fld.device, torch.float32)
            tgt = ((tgt[ss.perm] if ss.perm is not None else tgt) * ss.sw).contiguous()
            S.target = ptr(tgt)
        for d in range(fld.svh.depth):
            S.start[d], S.end[d] = ptr(st[d]), ptr(en[d])
        keep += [ss.xs, rows, st, en, tgt, ss.keys]
    return len(site_sets)


def _site_sets_and_structure(fld, hier, M, make_sets, too_large):
    """What both assemblies start with: the site sets (``make_sets(sets, keep)`` fills them and returns their number) and the
    structure pass -- own-upper counts and in-degrees of every row (nksr_assemble_count).  Returns (sets, nsets, keep, counts, ws,
    n_up, n_mir, nnz, td): keep holds every buffer the sets point into, counts [4, M + 1] = rowcount, crosscount, samelow, indeg
    (entry M of each is 0), ws is the workspace the fill shares with the pass, n_up / n_mir count the upper and the cross-level
    (mirrored) entries, nnz those of the whole matrix; td is the timing tick.  ``too_large``: the caller's message, with (M, nnz),
    for a system past 2^31 entries."""
    if M == 0:
        raise RuntimeError('empty hierarchy')
    keep = []  # keep every buffer alive until the launches are enqueued
    sets = (SiteSetT * 2)()
    nsets = make_sets(sets, keep)
    counts = torch.zeros((4, M + 1), dtype=torch.int32, device=fld.device)
    ws = torch.empty(int(_lib.lib.nksr_assemble_workspace_bytes(C.byref(hier))), dtype=torch.uint8, device=fld.device)
    td = _tick('_', time.perf_counter())
    call('nksr_assemble_count', C.byref(hier), ptr(ws), ptr(counts[0]), ptr(counts[1]), ptr(counts[2]), ptr(counts[3]), stream())
    n_up, n_mir = [int(v) for v in counts[:2].sum(dim=1, dtype=torch.int64).tolist()]
    td = _tick('asm:count', td)
    nnz = 2 * n_up + M
    if nnz >= 2 ** 31 - 4096:
        raise RuntimeError(too_large % (M, nnz))
    return sets, nsets, keep, counts, ws, n_up, n_mir, nnz, td


def _split_scratch(fld, hier):
    """(scratch or None, bytes): coarse cells hold thousands of site rows; with this scratch the levels that split and have few cells
    sum every cell's Gram block with several wavefronts (csrc/gram.hip).  Without it one wavefront per cell does: the same bits."""
    nbytes = int(_lib.lib.nksr_assemble_split_bytes(C.byref(hier)))
    return (torch.empty(nbytes, dtype=torch.uint8, device=fld.device) if nbytes else None), nbytes


def assemble(fld, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, reg_weight=1.0,
             pos_sorted_keys=None, normal_sorted_keys=None, coarse_from=None, fused_op=None):
    """Materialise the CSR normal equations.  Returns (rowptr, cols, vals, diag, b).
    ``*_sorted_keys``: level-0 Morton keys of site sets that are ALREADY Morton-sorted.
    ``coarse_from`` = c0: only the diagonal block of the levels >= c0 (plain CSR, local indices) -- the preconditioner's;
    with ``fused_op`` (fused_operator's result) it reads the kernel rows the matrix-free operator already holds."""
    dev = fld.device
    hier = fld._hier if coarse_from is None else fld._coarse_hier(int(coarse_from))
    M = fld.svh.num_unknowns if coarse_from is None else fld.svh.num_unknowns - fld.svh.offsets[int(coarse_from)]
    if fused_op is not None:
        def make_sets(sets, keep):
            return _sets_from_operator(fld, fused_op, coarse_from, sets, keep)
    else:
        def make_sets(sets, keep):
            return _sets_from_sites(fld, fld._site_sets((pos_xyz, None, pos_weight, pos_sorted_keys),
                                                        (normal_xyz, normal_value, normal_weight, normal_sorted_keys)), hier, sets, keep)
    # structure pass: own-upper counts + in-degrees -> exclusive scans -> final CSR row pointers
    sets, nsets, keep, counts, ws, n_up, n_mir, nnz, td = _site_sets_and_structure(
        fld, hier, M, make_sets, 'assembled system too large for one chunk (M=%d, nnz=%d >= 2^31): use the matrix-free solve '
        '(fused_mode=True) or pass chunk_size= to reconstruct() (examples/recons_by_chunk.py)')
    rowcount, crosscount, samelow, indeg = counts[0], counts[1], counts[2], counts[3]
    rowlen = indeg + samelow + rowcount + 1     # [cross-level mirrors][same-level lower][own upper][diagonal]
    rowlen[M] = 0
    rowptr = ops.exclusive_sum_i32(rowlen)
    mir_off = ops.exclusive_sum_i32(crosscount)
    mirptr = ops.exclusive_sum_i32(indeg)
    col_bits = ops._bits(M)
    # physical (tile-interleaved, zero-padded) CSR arrays for the streaming SpMV: packed 21-bit columns
    # (6.67 bytes per entry) whenever the unknowns fit, int32 columns otherwise (include/nksr_hip.h)
    fmt = 1 if M <= (1 << 21) and int(fld.solver_config.get('col_format', 1)) == 1 else 0
    if coarse_from is not None:
        fmt = 2
    chunk, tile = (4608, 192) if fmt == 1 else ((4096, 256) if fmt == 0 else (1, 1))
    npad = (nnz + chunk - 1) // chunk * chunk
    cols = torch.empty(npad, dtype=torch.int32, device=dev)
    vals = torch.empty(npad, dtype=torch.float32, device=dev)
    # only the pad must be zero (valid column 0, value 0); the last tile is interleaved, so its
    # unwritten slots are scattered through the whole tile: clear it from its start
    tail = nnz // tile * tile
    cols[tail:].zero_()
    vals[tail:].zero_()
    diag = torch.empty(M, dtype=torch.float32, device=dev)
    b = torch.empty(M, dtype=torch.float32, device=dev)
    mir_k = torch.empty(n_mir, dtype=torch.int64, device=dev)
    mir_v = torch.empty(n_mir, dtype=torch.float32, device=dev)
    split, split_bytes = _split_scratch(fld, hier)
    call('nksr_assemble', C.byref(hier), sets, nsets, float(reg_weight), col_bits, ptr(ws), ptr(rowptr), ptr(indeg),
         ptr(samelow), ptr(mir_off), fmt, ptr(cols), ptr(vals), ptr(diag), ptr(mir_k), ptr(mir_v), ptr(b), ptr(split), split_bytes, stream())
    td = _tick('asm:blocks+fill', td)
    del split
    del ws
    ks, vs = ops.sort_pairs(mir_k, mir_v.view(torch.int32), end_bit=col_bits)   # stable, destination-row bits only
    del mir_k, mir_v
    call('nksr_place_mirrors', ptr(ks), ptr(vs.view(torch.float32)), n_mir, col_bits, ptr(rowptr), ptr(mirptr), fmt, ptr(cols),
         ptr(vals), stream())
    del ks, vs
    td = _tick('asm:mirrors', td)
    if fmt == 1:
        packed = torch.empty(npad // 3, dtype=torch.int64, device=dev)
        call('nksr_pack_cols21', ptr(cols), npad, ptr(packed), stream())
        cols = packed
    if coarse_from is None:
        fld.nnz = nnz
    del keep
    return rowptr, cols, vals, diag, b


def assemble_packed(fld, reg_weight, coarse_from, fused_op, old_of_new, new_of_old, local_col, drop):
    """The packed (format 1) diagonal block of the levels >= ``coarse_from`` straight from the row fill (csrc/assemble.hip,
    nksr_assemble_packed; its rows: csrc/packed_rows.hip): the drop test runs where an entry is formed, so neither the fp32 CSR of the block nor the mirrors of the
    dropped entries exist.  ``old_of_new`` / ``new_of_old``: the segment-major renumbering (int32), ``local_col`` = new_of_old -
    seg_base[segment].  Returns (packed, packed_rowptr, dis, kept, nnz, diag): the arrays nksr_coarse_pack makes of the CSR, word for
    word, the structural entry count of the block, and its diagonal in the old order."""
    dev = fld.device
    c0 = int(coarse_from)
    hier = fld._coarse_hier(c0)
    M = fld.svh.num_unknowns - fld.svh.offsets[c0]
    sets, nsets, keep, counts, ws, n_up, n_mir, nnz, td = _site_sets_and_structure(
        fld, hier, M, lambda sets, keep: _sets_from_operator(fld, fused_op, c0, sets, keep), 'coarse block too large (M=%d, nnz=%d >= 2^31)')
    rowcount, crosscount, samelow = counts[0], counts[1], counts[2]
    own_off = ops.exclusive_sum_i32(samelow + rowcount)        # (entry M of both is 0)
    mir_off = ops.exclusive_sum_i32(crosscount)
    own = torch.empty(max(2 * n_up - n_mir, 1), dtype=torch.int32, device=dev)     # same-level lower (= same-level upper) + own upper
    mir = torch.empty(max(n_mir, 1), dtype=torch.int64, device=dev)
    kept = torch.empty((3, M + 1), dtype=torch.int32, device=dev)
    kept[:, M] = 0
    diag = torch.empty(M, dtype=torch.float32, device=dev)
    split, split_bytes = _split_scratch(fld, hier)
    call('nksr_assemble_packed', C.byref(hier), sets, nsets, float(reg_weight), ptr(ws), ptr(samelow), ptr(mir_off), ptr(own_off),
         ptr(new_of_old), ptr(local_col), float(drop), ptr(diag), ptr(own), ptr(mir), ptr(kept), ptr(split), split_bytes, stream())
    td = _tick('asm:blocks+fill', td)
    del split, ws, keep
    kept_off = ops.exclusive_sum_i32(kept[2])
    n_kept_mir = int(kept_off[M].item())
    dense = torch.empty(n_kept_mir, dtype=torch.int64, device=dev)
    if n_kept_mir:
        call('nksr_packed_mirrors_compact', M, ptr(mir), ptr(mir_off), ptr(kept[2]), ptr(kept_off), ptr(dense), stream())
    del mir
    srt = ops.sort_keys(dense, begin_bit=32, end_bit=32 + ops._bits(M))          # stable, destination-row bits only
    del dense
    runs = torch.empty(2 * M, dtype=torch.int32, device=dev)
    lens = torch.empty(M + 1, dtype=torch.int32, device=dev)
    lens[M:] = 0
    call('nksr_packed_row_lengths', M, ptr(srt), n_kept_mir, ptr(kept), ptr(old_of_new), ptr(runs), ptr(lens), stream())
    prow = ops.exclusive_sum_i32(lens)
    n_kept = int(prow[M].item())
    packed = torch.empty(max(n_kept, 1), dtype=torch.int32, device=dev)
    dis = torch.empty(M, dtype=torch.float32, device=dev)
    call('nksr_packed_rows', M, ptr(srt), ptr(runs), ptr(own), ptr(own_off), ptr(samelow), ptr(kept), ptr(old_of_new), ptr(prow),
         ptr(diag), ptr(packed), ptr(dis), stream())
    td = _tick('asm:mirrors+pack', td)
    return packed, prow, dis, n_kept, nnz, diag
