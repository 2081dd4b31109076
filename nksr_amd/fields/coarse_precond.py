"""Block preconditioner of the coarse levels of a KernelField's normal equations (nksr_coarse_precond_t, csrc/cheb.hip): the
diagonal block of the levels >= c0 as a small CSR, packed where it fits, and the Chebyshev interval of every segment's block."""
import ctypes as C
import os
import time

import torch

from .. import ops
from . import assembly
from .._lib import PC_MAX_STEPS, CoarsePrecondT, call, ptr, stream
from ._timing import _tick

PC_RATIO = 40.0          # Chebyshev interval [lambda_max / PC_RATIO, lambda_max] of the coarse block (100 until late round 3: 11.16 -> 10.9
#                          PCG iterations per chunk of the 64-chunk scene at the same step count; 10..20 are worse again, 200 much worse)
PC_DROP_TOL = 0.005        # packed coarse block: off-diagonal entries below this fraction of the (unit) diagonal are left out


def _renumber(n, row_seg, counts):
    """The segment-major order of the coarse unknowns: (old_of_new, new_of_old, seg_base, row_seg in the new order), all int32.
    It depends on ``row_seg`` alone, so it is known before the block is assembled."""
    ar = torch.arange(n, dtype=torch.int64, device=row_seg.device)
    old_of_new = torch.argsort(row_seg.long() * n + ar)
    new_of_old = torch.empty_like(old_of_new)
    new_of_old[old_of_new] = ar
    seg_base = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
    return old_of_new.to(torch.int32), new_of_old.to(torch.int32), seg_base, row_seg[old_of_new].contiguous()


def _pack_block(rowptr, cols, vals, diag, n, row_seg, counts, drop):
    """The block in packed form (csrc/cheb.hip, format 1): rows regrouped by segment, Jacobi-scaled half-precision values + 16-bit
    segment-local columns, off-diagonal entries below ``drop`` of the unit diagonal left out."""
    dev = rowptr.device
    o2n, n2o, seg_base, row_seg_new = _renumber(n, row_seg, counts)
    lens = torch.empty(n + 1, dtype=torch.int32, device=dev)
    lens[n:] = 0
    call('nksr_coarse_pack_count', ptr(rowptr), ptr(cols), ptr(vals), ptr(diag), n, ptr(o2n), drop, ptr(lens), stream())
    prow = ops.exclusive_sum_i32(lens)
    kept = int(prow[n].item())
    packed = torch.empty(max(kept, 1), dtype=torch.int32, device=dev)
    dis = torch.empty(n, dtype=torch.float32, device=dev)
    call('nksr_coarse_pack', ptr(rowptr), ptr(cols), ptr(vals), ptr(diag), n, ptr(o2n), ptr(n2o), ptr(row_seg_new), ptr(seg_base), ptr(prow),
         drop, ptr(packed), ptr(dis), stream())
    return packed, prow, dis, o2n, seg_base, row_seg_new, kept


def coarse_precond(fld, op, reg_weight, segments=None, sites=None, override=None):
    """Block preconditioner of the coarse levels (nksr_coarse_precond_t, csrc/cheb.hip): the diagonal block of the levels >= c0
    assembled as a small plain CSR + the largest Jacobi-scaled eigenvalue of every segment's block (left on the device: no
    host sync).  solver_config['coarse_precond']: None = automatic (see solve_fused), False = off, or a dict
    {'first_level', 'steps', 'ratio', 'packed', 'drop', 'direct'}."""
    cfg = fld.solver_config.get('coarse_precond')
    L = fld.svh.depth
    if cfg is False:
        return None
    cfg = dict(cfg) if isinstance(cfg, dict) else dict(override or {})
    for k, e in (('first_level', 'NKSR_PC_LEVEL'), ('steps', 'NKSR_PC_STEPS'), ('ratio', 'NKSR_PC_RATIO')):      # tuning knobs
        if e in os.environ and k not in cfg:
            cfg[k] = float(os.environ[e])
    c0 = int(cfg.get('first_level', 2))
    off = fld.svh.offsets
    M = fld.svh.num_unknowns
    if not 0 < c0 < L or M - off[c0] < 1:
        return None
    n = M - off[c0]
    nseg = segments.nseg if segments is not None else 1
    td = _tick('_', time.perf_counter())
    row_seg = segments.unknown_seg[off[c0]:].contiguous() if segments is not None else None
    # packed form (csrc/cheb.hip, format 1): Jacobi-scaled half-precision values + 16-bit segment-local columns, 4 bytes per entry
    # instead of 8 -- when every segment holds fewer than 2^16 coarse unknowns (chunks do; a large single field does not).  That
    # depends on row_seg alone: decided here, ahead of the assembly, which then emits the packed words itself (no fp32 CSR)
    rs = row_seg if row_seg is not None else torch.zeros(n, dtype=torch.int32, device=fld.device)
    counts = torch.bincount(rs.long(), minlength=nseg)
    pack = bool(cfg.get('packed', os.environ.get('NKSR_PC_PACKED', '1') != '0')) and int(counts.max()) < 65536
    drop = float(cfg.get('drop', os.environ.get('NKSR_PC_DROP', PC_DROP_TOL)))
    direct = pack and op is not None and bool(cfg.get('direct', True))      # ('direct': False = through the fp32 CSR and nksr_coarse_pack: the reference of the tests)
    if direct:              # from the kernel rows the matrix-free operator already holds, straight into the packed words
        o2n, n2o, seg_base, row_seg_new = _renumber(n, rs, counts)
        local = (n2o - seg_base[rs.long()]).contiguous()
        packed, prow, dis, kept, nnz, _ = assembly.assemble_packed(fld, reg_weight, c0, op, o2n, n2o, local, drop)
    elif op is not None:
        rowptr, cols, vals, diag, _ = fld.assemble(None, None, None, 1.0, 1.0, reg_weight, coarse_from=c0, fused_op=op)
    else:                   # the assembled solve: the same block from the site sets (rows of the masked hierarchy)
        rowptr, cols, vals, diag, _ = fld.assemble(reg_weight=reg_weight, coarse_from=c0, **sites)
    td = _tick('pc:assemble', td)
    lam = torch.empty(nseg, dtype=torch.float32, device=fld.device)
    coef = torch.empty(nseg * (1 + 2 * PC_MAX_STEPS), dtype=torch.float32, device=fld.device)
    pc = CoarsePrecondT()
    # the interval's upper end: 1.1 x the power-iteration estimate (a LOWER bound of lambda_max, within ~1 % after 8 steps), capped by
    # the Gershgorin bound (a true upper bound, 2-3x too large to be used by itself).  'lambda_scale' is a test knob: < 1 forces the
    # polynomial to lose definiteness, which the PCG answers by restarting the segment with Jacobi alone (csrc/pcg.hip)
    pc.first, pc.n, pc.steps, pc.lambda_scale, pc.ratio = off[c0], n, int(cfg.get('steps', 8)), float(cfg.get('lambda_scale', 1.1)), float(cfg.get('ratio', PC_RATIO))
    gersh = torch.empty(nseg, dtype=torch.float32, device=fld.device)
    pc.lambda_, pc.coef = ptr(lam), ptr(coef)
    if not direct:
        nnz = int(cols.numel())
    info = {'first_level': c0, 'unknowns': n, 'nnz': nnz, 'steps': int(pc.steps), 'lambda': lam}
    if pack:
        if not direct:
            packed, prow, dis, o2n, seg_base, row_seg_new, kept = _pack_block(rowptr, cols, vals, diag, n, rs, counts, drop)
        info.update(nnz_kept=kept + n, drop=drop)
        work = torch.empty(4 * n, dtype=torch.float32, device=fld.device)
        # ten steps instead of eight on large blocks: a packed step costs a third of a plain one (four rows per wavefront, half the
        # bytes, no tails), and every PCG iteration saved is a sweep over all kernel rows (configs[4], one GPU, ratio 40:
        # 8 / 10 / 12 steps -> 11.19 / 10.91 / 10.72 iterations per chunk, 390.7 / 392.5 / 395.7 ms per step: flat);
        # small blocks are bound by the number of launches, not by bytes: they keep eight
        # (chunk mode always takes ten: the count must not depend on how many chunks share the batch -- a chunk's iterates are
        # the same bits alone and among 63 others, tests/test_gpu_full_size.py)
        if 'steps' not in cfg and (segments is not None or n >= 100000):
            pc.steps = 10
            info['steps'] = 10
        pc.format, pc.row_seg, pc.work = 1, ptr(row_seg_new), ptr(work)
        pc.packed, pc.packed_rowptr, pc.dis, pc.old_of_new, pc.seg_base = ptr(packed), ptr(prow), ptr(dis), ptr(o2n), ptr(seg_base)
        call('nksr_coarse_lambda_max_packed', C.byref(pc), nseg, 8, ptr(work), ptr(lam), stream())
        call('nksr_coarse_gershgorin', C.byref(pc), nseg, ptr(work), ptr(gersh), stream())
        pc.gersh = ptr(gersh)
        info.update(packed=True, gershgorin=gersh, keep=(packed, prow, dis, o2n, seg_base, row_seg_new, work, lam, coef, gersh))
        td = _tick('pc:pack+lambda', td)
        return dict(info, pc=pc)
    work = torch.empty(3 * n, dtype=torch.float32, device=fld.device)
    # eight power-iteration steps from the all-ones vector land within ~1 % (measured): 10 % margin.  A segment whose block is
    # degenerate (no constraint rows on these levels: lambda <= 0) keeps Jacobi -- decided on the device (k_cheb_coeffs)
    call('nksr_coarse_lambda_max', ptr(rowptr), ptr(cols), ptr(vals), ptr(diag), n, 8, ptr(work), ptr(lam),
         C.byref(segments.c) if segments is not None else None, off[c0], stream())
    pc.format, pc.row_seg, pc.work = 0, ptr(row_seg), ptr(work)
    pc.rowptr, pc.cols, pc.vals, pc.diag = ptr(rowptr), ptr(cols), ptr(vals), ptr(diag)
    call('nksr_coarse_gershgorin', C.byref(pc), nseg, ptr(work), ptr(gersh), stream())
    pc.gersh = ptr(gersh)
    info.update(packed=False, gershgorin=gersh, keep=(rowptr, cols, vals, diag, work, lam, coef, row_seg, gersh))
    return dict(info, pc=pc)
