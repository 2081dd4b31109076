"""The chunked reconstruction as a sequence of phases: scene box, chunk plan, chunk inputs, batch plan, batched solves, halo
exchange.  ``reconstruct_by_chunk`` calls them in this order and wraps the parts into a ``MultiChunkField``."""
import os
import time
import types

import numpy as np
import torch
import torch.distributed as dist

from .. import dist as D
from .. import ops
from ..density import bbox_center
from ..fields.mask_fields import LayerField
from ..normals import TooFewPoints as ChunkTooSmall      # a normal-estimating preprocess_fn on a chunk with fewer points than k: chunk skipped
from .field import MultiChunkField
from .geometry import (MIN_CHUNK_POINTS, ChunkFrame, chunk_geometry, chunk_grid, chunk_grid_struct, chunk_index, chunk_pairs, exchange_band,
                       halo_destinations, halo_inner)
from .payload import ChunkPart, fields_from_payloads
from .residency import spill_to_disk


def select_chunk_points(xyz, lo, grid, chunk_size, band, wanted):
    """(point index, chunk id) of every point inside core +- band of a chunk in ``wanted`` (bool per chunk), sorted by
    (chunk, point index), + the points per chunk.  Same comparisons as a per-chunk boolean mask: x >= lo_c - band and
    x < hi_c + band along the split axes, the bounds rounded to fp32."""
    dev = xyz.device
    n = xyz.shape[0]
    nchunk = grid[0] * grid[1] * grid[2]
    z = torch.zeros(0, dtype=torch.long, device=dev)
    if n == 0:
        return z, z, [0] * nchunk
    G, keep = chunk_grid_struct(lo, grid, chunk_size, band, None, dev)
    flag = torch.tensor([0 if w else -1 for w in wanted], dtype=torch.int32, device=dev)
    _, idx, cid, _, _ = chunk_pairs(G, 0, xyz.contiguous(), flag, False)
    m = idx.shape[0]
    if m == 0:
        return z, z, [0] * nchunk
    cid = cid.long()
    if nchunk > 1:
        # the fill order is (point, chunk): a STABLE sort on the chunk bits alone gives (chunk, point) -- one radix pass over 6-8 bits
        ks, order = ops.sort_pairs(cid, torch.arange(m, dtype=torch.int32, device=dev), end_bit=ops._bits(nchunk))
        order = order.long()
        idx, cid = idx[order], ks
    counts = torch.bincount(cid, minlength=nchunk).tolist()
    return idx, cid, counts


def scene_box(xyz, chunk_bounds, collective, dev):
    """Phase 1.  Reads the cloud (finite check on its bounding box: nksr_bbox gives NaN in lo[0] when any coordinate is NaN /
    infinite, the CPU branch the extrema themselves).  Returns (lo[3], hi[3]) of the scene as floats: ``chunk_bounds``, else the
    local box, else -- ``collective`` -- the all_reduce of the ranks' boxes (a rank without points contributes +-inf)."""
    if xyz.shape[0]:
        lo_t, hi_t, _ = bbox_center(xyz)
        if not bool(torch.isfinite(torch.cat([lo_t.reshape(-1), hi_t.reshape(-1)])).all()):
            raise RuntimeError('non-finite coordinates in the input')
    else:
        lo_t = torch.full((3,), float('inf'), device=dev)
        hi_t = -lo_t
    if chunk_bounds is not None:
        return [float(v) for v in chunk_bounds[0]], [float(v) for v in chunk_bounds[1]]
    if collective:
        cd = D._comm_device(lo_t)
        lo_t, hi_t = lo_t.to(cd), hi_t.to(cd)
        dist.all_reduce(lo_t, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi_t, op=dist.ReduceOp.MAX)
    return [float(v) for v in lo_t.tolist()], [float(v) for v in hi_t.tolist()]


def chunk_plan(hp, xyz, lo, hi, chunk_size, overlap_ratio, rank, ws, collective, sharded_input, chunk_owner):
    """Phase 2.  Reads the scene box and the cloud (core of every point, one pass).  Returns the plan: ``lo``, ``chunk_size``,
    ``grid``, ``nchunk``, ``ov``, ``band``, ``frame``, ``cores`` {chunk: (lo[3], hi[3])}, ``counts`` (points per core -- the
    load-balance weights; all_reduce(MAX) of the ranks' counts when ``collective``), ``owner`` (``chunk_owner`` or
    dist.partition_chunks over ``world_size`` ranks) and ``jobs`` = this rank's chunks with a non-empty core (a chunk whose core is empty is skipped: the bands
    around it are covered by its neighbours' weights).  Raises when sharded input misses core points of an owned chunk."""
    grid = chunk_grid(lo, hi, chunk_size)
    ov, band = chunk_geometry(hp, chunk_size, overlap_ratio)
    frame = ChunkFrame(hp.voxel_size, hp.tree_depth, lo, grid, chunk_size, band)
    nchunk = grid[0] * grid[1] * grid[2]
    cores = {}
    for c in range(nchunk):
        clo = [lo[a] + ca * chunk_size for a, ca in enumerate(frame.chunk3(c))]
        cores[c] = (clo, [clo[a] + chunk_size for a in range(3)])
    counts_t = torch.bincount(chunk_index(xyz, lo, grid, chunk_size)[1], minlength=nchunk)
    local_counts = counts_t.tolist()
    counts = local_counts
    if collective:
        ct = counts_t.to(D._comm_device(counts_t))
        dist.all_reduce(ct, op=dist.ReduceOp.MAX)
        counts = ct.tolist()
    if chunk_owner is not None:
        if len(chunk_owner) != nchunk:
            raise RuntimeError('chunk_owner has %d entries, the chunk grid %s has %d chunks' % (len(chunk_owner), grid, nchunk))
        owner = [int(o) for o in chunk_owner]
    else:
        owner = D.partition_chunks(nchunk, ws, counts, grid)
    jobs = [c for c in range(nchunk) if owner[c] == rank and counts[c] > 0]
    for c in jobs:
        if sharded_input and local_counts[c] != counts[c]:
            raise RuntimeError('sharded input: rank %d owns chunk %d but holds %d of its %d core points' % (rank, c, local_counts[c], counts[c]))
    return types.SimpleNamespace(lo=lo, chunk_size=chunk_size, grid=grid, nchunk=nchunk, ov=ov, band=band, frame=frame, cores=cores,
                                 counts=counts, owner=owner, world_size=ws, jobs=jobs)


def chunk_inputs(plan, xyz, normal, sensor, preprocess_fn):
    """Phase 3.  Reads the cloud and the plan's jobs.  Returns (positions, normals, chunk id per point, points per chunk, jobs): the
    points inside core +- band of every job, sorted by chunk, each chunk passed through ``preprocess_fn`` on its own; the jobs left
    after dropping the chunks that ended below MIN_CHUNK_POINTS (or raised ChunkTooSmall), in slot order."""
    dev, nchunk = xyz.device, plan.nchunk
    mine = set(plan.jobs)
    pidx, pcid, npts = select_chunk_points(xyz, plan.lo, plan.grid, plan.chunk_size, plan.band, [c in mine for c in range(nchunk)])
    bx, bn, bc = xyz[pidx], (normal[pidx] if normal is not None else None), pcid
    if preprocess_fn is not None:
        # the reference's contract: preprocess_fn sees the points of ONE chunk, in the caller's coordinates, on the calling thread
        xs_, ns_, cs_ = [], [], []
        bs = sensor[pidx] if sensor is not None else None
        o = 0
        for c in range(nchunk):
            m = npts[c]
            if m == 0:
                continue
            sl = slice(o, o + m)
            o += m
            try:
                cx_, cn_, _ = preprocess_fn(bx[sl].contiguous(), bn[sl].contiguous() if bn is not None else None,
                                            bs[sl].contiguous() if bs is not None else None)
            except ChunkTooSmall:
                npts[c] = 0
                continue
            if cn_ is None:
                raise RuntimeError('oriented input required (normal= or sensor= with a normal-estimating preprocess_fn)')
            npts[c] = int(cx_.shape[0])
            xs_.append(cx_)
            ns_.append(cn_.to(torch.float32))
            cs_.append(torch.full((cx_.shape[0],), c, dtype=torch.long, device=dev))
        bx = torch.cat(xs_) if xs_ else xyz[:0]
        bn = torch.cat(ns_) if ns_ else xyz[:0]
        bc = torch.cat(cs_) if cs_ else pcid[:0]
    if bn is None:
        raise RuntimeError('oriented input required (normal= or sensor= with a normal-estimating preprocess_fn)')
    small = [c for c in plan.jobs if npts[c] < MIN_CHUNK_POINTS]          # a handful of stray points: nothing to solve, neighbours cover the band
    if small:
        keep = torch.ones(nchunk, dtype=torch.bool, device=dev)
        keep[small] = False
        s = torch.nonzero(keep[bc]).reshape(-1)
        bx, bn, bc = bx[s], bn[s], bc[s]
        for c in small:
            npts[c] = 0
    # (non-finite normals: caught by the box readback every batch starts with, Reconstructor._key_bits)
    jobs = sorted((c for c in plan.jobs if npts[c] >= MIN_CHUNK_POINTS), key=lambda c: plan.frame.key_range(c)[0])
    return bx, bn, bc, npts, jobs


def batch_budget(rec, fused_mode):
    """Phase 4a.  Points per batched solve: ``rec.chunk_batch_points``, else as many as the FREE memory of the device holds (the
    reference's chunk mode exists to bound memory, examples/recons_by_chunk.py:17-18) -- at most 2^25 points.  A batched solve takes
    ~4.5 KB of HBM per solved point at tree_depth 5 (84.7 GB for the 19.7 M band-included points of the 64-chunk scene; kernel rows
    are 45 % of it), in proportion to the depth; 70 % of what is free (+ what torch's allocator holds unused) may be planned with.
    0 for the assembled solve (fused_mode=False), which has no segmented form: one chunk per solve, as the reference runs them."""
    if not fused_mode:
        return 0
    budget = int(getattr(rec, 'chunk_batch_points', 0) or 0)
    if budget > 0:
        return budget
    budget, dev = 1 << 25, rec.device
    if dev.type == 'cuda':
        free = float(os.environ.get('NKSR_FREE_HBM_GB', 0)) * 1e9
        if free <= 0:
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        # (factor records are a fifth of the rows, but the set-up sweep holds the dense rows of the coarse levels beside them: peak ~0.9)
        factors = str(getattr(rec, 'row_format', None) or os.environ.get('NKSR_ROW_FORMAT')) == 'factors'
        per_point = 4500.0 * rec.hparams.tree_depth / 5.0 * (0.9 if factors else 1.0)
        budget = int(max(min(budget, 0.7 * free / per_point), 1))
    return budget


def plan_batches(jobs, npts, budget):
    """Phase 4b.  Sub-batches of whole chunks, ``jobs`` kept in their (slot) order: a batch is closed when the next chunk would take
    it past ``budget`` points, so a chunk larger than the budget goes alone and budget 0 gives one chunk per batch.  Results do not
    depend on the split (tests/test_gpu_full_size.py: a chunk alone == the chunk in the batch, bit for bit)."""
    batches, cur, acc = [], [], 0
    for c in jobs:
        if cur and acc + npts[c] > budget:
            batches.append(cur)
            cur, acc = [], 0
        cur.append(c)
        acc += npts[c]
    if cur:
        batches.append(cur)
    return batches


def solve_batches(rec, plan, batches, bx, bn, bc, approx_kernel_grad, solver_max_iter, solver_tol, fused_mode, park):
    """Phase 5.  Reads the chunk inputs and the batches.  Every batch is translated into the exploded frame (x' = x + T_c, one fp32
    rounding), checked against its slots and solved as one cloud (Reconstructor._reconstruct_single); with ``park`` and several
    batches a solved batch moves to ``rec.chunk_tmp_device`` (the reference's semantics) and on to ``rec.chunk_spill_dir``.  Returns
    ([ChunkPart per batch], timing: the stage times summed over the batches + 'spilled_bytes')."""
    frame, nchunk, dev = plan.frame, plan.nchunk, rec.device
    shift_all = torch.from_numpy(np.stack([frame.shift(c) for c in range(nchunk)])).to(dev)
    slot_org = torch.from_numpy(np.stack([np.asarray(frame.slot_origin(c), np.float64) * frame.w0 for c in range(nchunk)]).astype(np.float32)).to(dev)
    parts, timing = [], {}
    for ids in batches:
        if len(batches) > 1:
            inb = torch.zeros(nchunk, dtype=torch.bool, device=dev)
            inb[ids] = True
            s = torch.nonzero(inb[bc]).reshape(-1)
            x_b, n_b, c_b = bx[s], bn[s], bc[s]
        else:
            x_b, n_b, c_b = bx, bn, bc
        xs = (x_b + shift_all[c_b]).contiguous()
        rlo, rhi, _ = bbox_center((xs - slot_org[c_b]).contiguous())
        rlo, rhi = rlo.tolist(), rhi.tolist()
        if min(rlo) < frame.usable_lo or max(rhi) >= frame.usable_hi:
            raise RuntimeError('chunk data leaves its slot of the exploded frame (extent %s .. %s, usable %.3f .. %.3f): points outside '
                               'chunk_bounds along an axis that is not split?' % (rlo, rhi, frame.usable_lo, frame.usable_hi))
        kr = [frame.key_range(c) for c in ids]
        fld = rec._reconstruct_single(xs, n_b.to(torch.float32).contiguous(), approx_kernel_grad, solver_max_iter, solver_tol, fused_mode,
                                      chunks=(ids, [k[0] for k in kr], [k[1] for k in kr], frame) if fused_mode else None)
        fld.matrix = None
        fld._fused_op = None
        for k, v in getattr(fld, 'timing', {}).items():
            timing[k] = timing.get(k, 0.0) + v
        if park and rec.chunk_tmp_device != dev and len(batches) > 1:
            fld.to_(rec.chunk_tmp_device)
            if getattr(rec, 'chunk_spill_dir', None) and torch.device(rec.chunk_tmp_device).type == 'cpu':
                timing['spilled_bytes'] = timing.get('spilled_bytes', 0) + spill_to_disk(fld, rec.chunk_spill_dir)
        parts.append(ChunkPart(fld, ids, frame))
    return parts, timing


def exchange_halos(rec, plan, parts, timing, inner, exchange):
    """Phase 6.  Reads the solved parts.  ``exchange(local, dest_of) -> payload`` (dist.exchange_payloads_to, a simulation of it, or
    None: a single process) carries the HALO of every solved chunk -- the voxels other ranks can touch (exchange_band), not the whole
    field -- to the ranks that need it; which chunks were actually solved travels with it (a sparse chunk may have been skipped by
    its owner).  Appends the part made of the halos received and sets timing['t_exchange'] (pack, size + byte collectives, the remote
    field's tables)."""
    t_x = _now(rec)          # (taken also without an exchange: with sync_timing the solves are waited for here)
    if exchange is None:
        return
    hp, frame = rec.hparams, plan.frame
    local = {}
    for p in parts:
        local.update(p.pack_halos({c: exchange_band(plan.cores[c], frame.chunk3(c), plan.grid, plan.ov, hp.voxel_size, inner) for c in p.ids}))
    # a rank only evaluates the blend inside its own cores (+ the halo ring it evaluates): it needs exactly the chunks whose
    # weight support (core +- ov) reaches there -- its spatial neighbours, not all N.  Who needs what is geometry (cores, owners,
    # which cores hold points): every rank computes the same table, so a halo is SENT only to the ranks that need it
    # (all_to_all with per-pair sizes; a chunk its owner skipped is simply not sent)
    dest_of = halo_destinations(plan.cores, plan.ov + inner, plan.grid, plan.owner, plan.counts, plan.world_size)
    payload = exchange(local, dest_of)
    need = sorted((c for c in payload if c not in local), key=lambda c: frame.key_range(c)[0])
    if need:
        remote = fields_from_payloads([(frame.key_range(c)[0], payload[c][0], payload[c][1]) for c in need], hp.voxel_size, rec.network.interpolators,
                                      rec.device)
        remote.meshing_depth = int(hp.adaptive_depth)
        if remote.mask_field is None:
            remote.set_mask_field(LayerField(remote.svh, hp.adaptive_depth))
        parts.append(ChunkPart(remote, need, frame, solved=False))
    timing['t_exchange'] = _now(rec) - t_x


def reconstruct_by_chunk(rec, xyz, normal, sensor, chunk_size, overlap_ratio, approx_kernel_grad, solver_max_iter,
                         solver_tol, fused_mode, preprocess_fn, sim=None, sharded_input=False, chunk_owner=None, chunk_bounds=None, sim_exchange=None):
    """``sim=(rank, world_size)`` runs one simulated rank without a process group (tests); with ``sim_exchange(local, dest_of) ->
    payload`` the simulated rank goes through the halo exchange step too, the callable standing in for the collectives
    (tools/prof_rank_tail.py: everything a rank of N does after its solve, timed on one GPU).
    ``sharded_input``: every rank passes only ITS part of the cloud -- at least the points inside core +- band of the
    chunks it owns ("each rank receives only its chunks' points (+overlap)").  The chunk grid then
    comes from ``chunk_bounds`` = (lo[3], hi[3]) or from an all_reduce of the local bounding boxes, the per-core point
    counts from an all_reduce(MAX) (some rank holds every core completely), and ``chunk_owner`` (list, one rank per
    chunk) lets the caller that distributed the data dictate the ownership it assumed."""
    hp, dev = rec.hparams, rec.device
    rank, ws = sim if sim is not None else D.world()
    active = D.active() and sim is None            # a process group takes part (world > 1, or forced at world 1: NKSR_DIST_FORCE)
    collective = sharded_input and active
    lo, hi = scene_box(xyz, chunk_bounds, collective, dev)
    plan = chunk_plan(hp, xyz, lo, hi, chunk_size, overlap_ratio, rank, ws, collective, sharded_input, chunk_owner)
    bx, bn, bc, npts, jobs = chunk_inputs(plan, xyz, normal, sensor, preprocess_fn)
    batches = plan_batches(jobs, npts, batch_budget(rec, fused_mode))
    parts, timing = solve_batches(rec, plan, batches, bx, bn, bc, approx_kernel_grad, solver_max_iter, solver_tol, fused_mode,
                                  park=not active and sim is None)
    rec.timing = timing
    inner = halo_inner(hp.voxel_size, hp.adaptive_depth, getattr(rec, 'dual_graph', 'lattice'))      # how deep a halo reaches into its own core
    exchange = D.exchange_payloads_to if active else sim_exchange if sim is not None else None
    exchange_halos(rec, plan, parts, timing, inner, exchange)
    # (batches parked on chunk_tmp_device stay there: the blend borrows one part at a time -- borrowed() -- so meshing a scene
    # whose chunks do not fit the GPU together works as the reference's small-memory recipe says, NKSR-USAGE.md:150-167)
    mf = MultiChunkField(parts, plan.cores, plan.ov, lo, chunk_size, plan.grid, plan.owner, rank, ws, plan.frame, rec.network.interpolators, dev,
                         distributed=active, adaptive_depth=int(hp.adaptive_depth), halo_inner=inner)
    mf.dual_graph = getattr(rec, 'dual_graph', 'lattice')
    return mf


def _now(rec):
    if getattr(rec, 'sync_timing', False):
        torch.cuda.current_stream().synchronize()
    return time.perf_counter()
