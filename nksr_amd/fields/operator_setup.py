"""Set-up of the matrix-free operator of a KernelField (csrc/fused_tables.hip, fused_sweep.hip, fused.hip; nksr_fused_op_t), in four steps: the site sets
(KernelField._site_sets, shared with the assembly), the row layout, the row fill and the operator's tables."""
import ctypes as C
import os
import time

import torch

from .. import _lib, ops
from .._lib import FusedOpT, call, ptr, stream
from ._timing import _tick
from .row_layout import first_rows_from_ranks, pad_segments


def _first_rows_by_sort(sets):
    """NKSR_ROW_ORDER=sort: the unpadded first rows from a radix sort of the concatenated keys, a scan and a scatter -- what a test
    pins the rank passes of row_layout() against."""
    dev = sets[0].xs.device
    counts = [s.xs.shape[0] for s in sets]
    nsite = sum(counts)
    _, order = ops.sort_pairs(torch.cat([s.keys for s in sets]), torch.arange(nsite, dtype=torch.int32, device=dev), level=0)
    rows_site = torch.cat([torch.full((n,), s.rows, dtype=torch.int32, device=dev) for n, s in zip(counts, sets)])
    order = order.long()
    first_row = ops.exclusive_sum_i32(torch.cat([rows_site[order], rows_site.new_zeros(1)]))       # [nsite + 1]
    row_of_site = torch.empty(nsite, dtype=torch.int32, device=dev)
    row_of_site[order] = first_row[:nsite]
    return list(torch.split(row_of_site, counts))


def row_layout(sets, segments=None):
    """ONE Morton-ordered row list for all site sets (the stable merge of the sites' level-0 keys; a position site owns one row, a
    normal site three or four): the rows of a cell -- of both sets -- are then one contiguous run at every level.
    Returns (first row of every site per set, rows_total, pad_rows, item_seg); the last two are None without segments."""
    dev = sets[0].xs.device
    if os.environ.get('NKSR_ROW_ORDER', 'merge') == 'sort':
        first = _first_rows_by_sort(sets)
    elif len(sets) == 1:
        first = [torch.arange(sets[0].xs.shape[0], dtype=torch.int32, device=dev) * sets[0].rows]
    else:
        # Both site lists are sorted already: the merged order is a MERGE, and all it is needed for is every site's first row --
        # two rank passes (nksr_rank_sorted) instead of a 63-bit radix sort of the concatenated keys, a scan and a scatter
        (ka, na), (kb, nb) = [(s.keys, s.xs.shape[0]) for s in sets]
        ra = torch.empty(na, dtype=torch.int32, device=dev)
        rb = torch.empty(nb, dtype=torch.int32, device=dev)
        call('nksr_rank_sorted', ptr(kb), nb, ptr(ka), na, 0, ptr(ra), stream())          # sites of set 1 with a smaller key
        call('nksr_rank_sorted', ptr(ka), na, ptr(kb), nb, 1, ptr(rb), stream())          # sites of set 0 with a smaller or equal key
        first = list(first_rows_from_ranks(na, nb, ra, rb, sets[0].rows, sets[1].rows))
    rows_total, pad_rows, item_seg = sum(s.xs.shape[0] * s.rows for s in sets), None, None
    if segments is not None:
        first, rows_total, pad_rows, item_seg = pad_segments(first, [s.keys for s in sets], [s.rows for s in sets], segments)
    return [f.contiguous() for f in first], rows_total, pad_rows, item_seg


def alloc_rows(fld, sets, first_rows, rows_total, pad_rows, fac):
    """The row arrays (readable past the end: the operator's loads are unconditional, the last workgroup reads up to 255 + 63 rows
    past it), pad rows cleared, and -- where ONE launch writes the rows of both sets (kernel_dim 4, dense-slot rows; csrc/rows.hip:
    k_kernel_rows_merged -- the interleaved rows of two launches reach HBM as partial lines) -- the source site of every row.
    NKSR_ROWS_KERNEL=site keeps the launch per set (bit-identical rows)."""
    dev, L, M = fld.device, fld.svh.depth, fld.svh.num_unknowns
    R = {'rows_all': None, 'fac_vec': None, 'fac_pos': None, 'psi_all': None, 'merged': None, 'rows_total': rows_total}
    R['row_cells'] = torch.empty((L, rows_total), dtype=torch.int32, device=dev)
    R['targets_all'] = torch.zeros(rows_total + 320, dtype=torch.float32, device=dev)[:rows_total]
    if (not fac and fld.kdim == 4 and fld.hidden in (16, 32) and os.environ.get('NKSR_ROWS_KERNEL', 'merged') == 'merged'
            and max(s.xs.shape[0] for s in sets) < 2 ** 29):
        row_src = torch.full((rows_total,), -1, dtype=torch.int32, device=dev)
        args = {False: (None, None, 1.0), True: (None, None, 1.0)}           # (sites, per-site scale, scale) of the position / normal set
        for s, ri in zip(sets, first_rows):
            call('nksr_row_sources', ptr(ri), s.xs.shape[0], s.rows, int(s.grad), ptr(row_src), stream())
            args[s.grad] = (s.xs, s.site_scale, s.scale)
        R['merged'] = (row_src, args[False], args[True])
    if fac:
        fac_vec = R['fac_vec'] = torch.empty(L * rows_total * 4 + 320 * 4, dtype=torch.float32, device=dev)
        fac_vec[L * rows_total * 4:].zero_()
        fac_pos = R['fac_pos'] = torch.empty((rows_total + 320) * 4, dtype=torch.float32, device=dev)
        fac_pos[rows_total * 4:].zero_()
        R['psi_all'] = torch.cat([p.reshape(-1, 4) for p in fld._psi]).contiguous()
        assert R['psi_all'].shape[0] == M
    else:
        rows_all = R['rows_all'] = torch.empty(L * rows_total * 27 + 320 * 27, dtype=torch.float32, device=dev)
        rows_all[L * rows_total * 27:].zero_()
    if pad_rows is not None and pad_rows.numel():
        R['row_cells'][:, pad_rows] = -1
        if fac:
            fac_vec[:L * rows_total * 4].view(L, rows_total, 4)[:, pad_rows] = 0.0
            fac_pos[:rows_total * 4].view(rows_total, 4)[pad_rows] = 0.0                             # (kind 0: a position row without a cell)
        else:
            rows_all[:L * rows_total * 27].view(L, rows_total, 27)[:, pad_rows] = 0.0
    return R


def fill_rows(fld, sets, first_rows, R):
    """The kernel rows (pre-multiplied by sqrt(weight)) and their cells -- the merged launch, or a launch per set of the dense-slot
    rows or the factor records -- and the rows' targets."""
    dev, rows_total, row_cells = fld.device, R['rows_total'], R['row_cells']
    if R['merged'] is not None:
        # the rows' cells first (one pass, the probes of all levels in flight together): the row kernel then starts from them
        row_src, (xa, sa, fa), (xb, sb, fb) = R['merged']
        call('nksr_row_cells_merged', C.byref(fld._hier), ptr(xa), ptr(xb), ptr(row_src), rows_total, ptr(row_cells), stream())
        call('nksr_kernel_rows_merged', C.byref(fld._hier), ptr(xa), ptr(sa), float(fa), ptr(xb), ptr(sb), float(fb),
             int(fld.approx_kernel_grad), ptr(row_src), rows_total, ptr(row_cells), ptr(R['rows_all']), stream())
    for s, ri in zip(sets, first_rows):
        if R['merged'] is not None:
            pass
        elif R['fac_vec'] is not None:
            fld.kernel_factors_level_major(s.xs, s.grad, s.scale, R['fac_vec'], R['fac_pos'], rows_total, ri, row_cells, site_scale=s.site_scale)
        else:
            fld.kernel_rows_level_major(s.xs, s.grad, s.scale, R['rows_all'], rows_total, ri, row_cells, site_scale=s.site_scale)
        if s.target is not None:
            nc = 3 if s.grad else 1                                                                 # target components; the header row's is 0
            tgt = s.target.detach().to(dev, torch.float32)
            tgt = (tgt[s.perm] if s.perm is not None else tgt).reshape(s.xs.shape[0], nc)
            tgt = tgt * (s.sw[:, None] if torch.is_tensor(s.sw) else s.sw)                          # row order (site, component)
            R['targets_all'][(ri.long()[:, None] + (s.rows - nc) + torch.arange(nc, device=dev)[None]).reshape(-1)] = tgt.reshape(-1)


def operator_tables(fld, R, item_seg, segments):
    """Work items = runs of 32 rows, eight of them a workgroup of the sweep; a cell whose rows lie inside one workgroup is finished
    there, a cell that reaches into k > 1 workgroups owns k partial blocks (the coarse cells: ~1 % of all).  Returns the
    nksr_fused_op_t, span (first / last row of every cell, first workgroup), nblocks, n_multi, nnz_counter (one int64: the stored
    entries once nksr_fused_rhs_diag has run), nnz_scratch (the sweep's per-workgroup counts behind it) and the buffers to keep."""
    dev, L, M, rows_total = fld.device, fld.svh.depth, fld.svh.num_unknowns, R['rows_total']
    span = torch.empty((3, M), dtype=torch.int32, device=dev)
    counts = torch.empty(M + 1, dtype=torch.int32, device=dev)
    item_begin = torch.empty(int(_lib.lib.nksr_fused_item_entries(rows_total)), dtype=torch.int32, device=dev)
    nbr32 = torch.empty((M, 32), dtype=torch.int32, device=dev)
    nbrT = torch.empty((27, M), dtype=torch.int32, device=dev)
    call('nksr_fused_block_counts', L, M, rows_total, ptr(R['row_cells']), ptr(span), ptr(item_begin), ptr(counts), stream())
    offsets = ops.exclusive_sum_i32(counts)
    call('nksr_fused_tables', C.byref(fld._hier), rows_total, ptr(item_begin), ptr(offsets), ptr(span), ptr(nbr32), ptr(nbrT), stream())
    nblocks = int(offsets[M].item())
    big = torch.nonzero(counts[:M] > 16).reshape(-1).to(torch.int32)          # coarse cells: a workgroup each in the per-cell sum
    multi = torch.cat([big, torch.nonzero((counts[:M] > 1) & (counts[:M] <= 16)).reshape(-1).to(torch.int32)])
    ws = torch.empty(int(_lib.lib.nksr_fused_workspace_bytes(nblocks, M)), dtype=torch.uint8, device=dev)
    cell_sums = torch.zeros((27, M), dtype=torch.float32, device=dev)
    op = FusedOpT()
    op.depth, op.M, op.n_multi, op.n_big, op.rows_total, op.nblocks = L, M, int(multi.numel()), int(big.numel()), rows_total, nblocks
    op.rows_all, op.targets_all, op.row_cells = ptr(R['rows_all']), ptr(R['targets_all']), ptr(R['row_cells'])
    op.nbr32, op.nbrT, op.item_begin = ptr(nbr32), ptr(nbrT), ptr(item_begin)
    if R['fac_vec'] is not None:
        op.fac_vec, op.fac_pos, op.psi_all, op.inv_w0 = ptr(R['fac_vec']), ptr(R['fac_pos']), ptr(R['psi_all']), float(fld.svh.inv_w0)
    op.offsets, op.multi, op.workspace, op.cell_sums = ptr(offsets), (ptr(multi) if multi.numel() else None), ptr(ws), ptr(cell_sums)
    # SURVEY.md section 8d counts the operator's bytes per STORED entry; the dense-slot rows hold structural zeros (absent
    # neighbours, B-spline support ends): the set-up pass counts the non-zero slots on its way (read back on demand)
    # (word 0: the total; behind it the sweep's scratch, one count per workgroup, no initial value -- the sweep shares no word)
    nnz_words = torch.empty(int(_lib.lib.nksr_fused_count_words(rows_total)), dtype=torch.int64, device=dev)
    nnz_counter, nnz_scratch = nnz_words[:1], nnz_words[1:]
    nnz_counter.zero_()
    op.nnz_counter = ptr(nnz_words)
    keep = [nbr32, nbrT, item_begin, offsets, multi, ws, cell_sums, nnz_words]
    if item_seg is not None:
        op.item_seg, op.unknown_seg = ptr(item_seg), ptr(segments.unknown_seg)
        keep += [item_seg, segments.unknown_seg]
    return {'op': op, 'span': span, 'nblocks': nblocks, 'n_multi': int(multi.numel()), 'nnz_counter': nnz_counter, 'nnz_scratch': nnz_scratch,
            'keep': keep}


def fused_operator(fld, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, pos_sorted_keys=None, normal_sorted_keys=None,
                   pos_value=None, segments=None):
    """Everything the matrix-free operator needs (csrc/fused_sweep.hip, fused.hip; nksr_fused_op_t): the level-major kernel rows of both
    site sets in one array (pre-multiplied by sqrt(weight)), their targets, the global neighbour table and the work
    items.  Returns a dict; ``keep`` holds the buffers the C struct points into."""
    if fld.svh.num_unknowns == 0:
        raise RuntimeError('empty hierarchy')
    fac = fld._row_format() == 'factors'
    # (ROWS a normal site owns in the list: three -- or, in the factor form, four: a header row that carries phi and contributes
    # nothing, then one row per axis)
    sets = fld._site_sets((pos_xyz, pos_value, pos_weight, pos_sorted_keys), (normal_xyz, normal_value, normal_weight, normal_sorted_keys),
                          rows_per_normal=4 if fac else 3, per_site_weights=True)
    if not sets:
        raise RuntimeError('no constraint sites')
    first_rows, rows_total, pad_rows, item_seg = row_layout(sets, segments)
    td = _tick('_', time.perf_counter())
    R = alloc_rows(fld, sets, first_rows, rows_total, pad_rows, fac)
    td = _tick('op:alloc', td)
    fill_rows(fld, sets, first_rows, R)
    td = _tick('op:kernel_rows', td)
    T = operator_tables(fld, R, item_seg, segments)
    td = _tick('op:tables', td)
    T['keep'] += [R, first_rows] + [s.xs for s in sets]
    return dict(T, nsets=len(sets), rows_total=rows_total, rows_all=R['rows_all'], row_format='factors' if fac else 'dense',
                fac_vec=R['fac_vec'], fac_pos=R['fac_pos'], row_cells=R['row_cells'], targets_all=R['targets_all'],
                item_seg=item_seg, pad_rows=pad_rows)
