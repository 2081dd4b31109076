"""The chunk grid and the exploded frame: which chunk a point is in, where a chunk's slot lies, which chunks and ranks touch.
Host arithmetic, except ``chunk_grid_struct`` and ``chunk_pairs`` (the tables and the launches of csrc/chunks.hip)."""
import ctypes as C
import math

import numpy as np
import torch

from .. import dist as D
from .. import ops
from .._lib import ChunkGridT, call, ptr, stream


def chunk_grid(lo, hi, chunk_size):
    n = [max(1, int(math.ceil((hi[a] - lo[a]) / chunk_size - 1e-9))) for a in range(3)]
    return n


def chunk_index(xyz, origin, grid, chunk_size, offset=0.0):
    """([ix, iy, iz], linear id) of the chunk whose core holds ``xyz + offset``: (x + offset - origin) / chunk_size in fp32, rounded down, clamped
    to the grid (points outside the box belong to the border chunks), id = (ix * gy + iy) * gz + iz.  An axis that is not split
    contributes the integer 0.  ``ChunkFrame.chunk3`` is the inverse."""
    idx = []
    cid = torch.zeros(xyz.shape[0], dtype=torch.long, device=xyz.device)
    for a in range(3):
        ia = 0
        if grid[a] > 1:
            x = xyz[:, a] + offset if offset else xyz[:, a]
            ia = torch.floor((x - origin[a]) / chunk_size).long().clamp_(0, grid[a] - 1)
        idx.append(ia)
        cid = cid * grid[a] + ia
    return idx, cid


OV_FLOOR = 1.0        # blend half-width floor, in coarsest voxels
BAND_EXTRA = 1.5      # data margin beyond core +- ov, in coarsest voxels (= the support radius of the coarsest kernel); None = ov
MIN_CHUNK_POINTS = 8
SLOT_GAP = 6          # empty coarsest voxels between the data of two slots (kernel support 1.5 + structure dilation 1, both sides, + slack)


def chunk_geometry(hp, chunk_size, overlap_ratio):
    wc = hp.voxel_size * 2 ** (hp.tree_depth - 1)
    ov = max(overlap_ratio * chunk_size, OV_FLOOR * wc)
    band = 2 * ov if BAND_EXTRA is None else ov + BAND_EXTRA * wc
    return ov, band


class ChunkFrame:
    """Geometry of the exploded frame.  Chunk (cx, cy, cz) of the grid owns the cube [s * 2^S, (s + 1) * 2^S)^3 of the finest
    lattice, s = (cx, cy, cz) - grid // 2 (centred: small coordinates keep fp32 resolution); its data is translated by
    T_c = slot origin + low - a_c, a_c = the chunk's data corner rounded down to a multiple of 2^depth finest voxels, low = 4
    coarsest voxels -- a whole number of voxels at EVERY level, so the chunk's own lattice is kept.
    2^S >= low + data extent + alignment slack + SLOT_GAP / 2 coarsest voxels."""

    def __init__(self, voxel_size, depth, lo, grid, chunk_size, band):
        self.w0, self.depth = float(voxel_size), int(depth)
        self.lo, self.grid, self.chunk_size, self.band = [float(v) for v in lo], [int(g) for g in grid], float(chunk_size), float(band)
        self.align = 1 << self.depth
        # a chunk's voxels reach up to one coarsest voxel beyond its points (structure dilation) and its kernels 1.5 more: the data
        # sits `low` finest voxels (4 coarsest, a multiple of the alignment) inside its slot and ends >= SLOT_GAP / 2 coarsest
        # voxels before the slot's end, so that ALL voxels of a chunk lie inside its slot (= its Morton key range)
        self.low = 2 * self.align
        ext = int(math.ceil((self.chunk_size + 2 * self.band) / self.w0)) + 2
        need = self.low + ext + self.align + ((SLOT_GAP // 2) << (self.depth - 1))
        S = self.depth
        while (1 << S) < need:
            S += 1
        self.S = S
        self.half = [g // 2 for g in self.grid]
        reach = max(max(self.grid[a] - self.half[a], self.half[a]) for a in range(3)) << S
        if reach >= (1 << 20) - (1 << S):
            raise RuntimeError('chunk grid %s with %d-voxel slots does not fit the 2^20 lattice: use a larger chunk_size' % (self.grid, 1 << S))
        # data must stay inside [usable_lo, usable_hi) of its slot (model units)
        self.usable_lo = (self.low - 1) * self.w0
        self.usable_hi = ((1 << S) - ((SLOT_GAP // 2) << (self.depth - 1))) * self.w0

    def chunk3(self, c):
        g = self.grid
        return (c // (g[1] * g[2]), (c // g[2]) % g[1], c % g[2])

    def slot_origin(self, c):
        c3 = self.chunk3(c)
        return [(c3[a] - self.half[a]) << self.S for a in range(3)]

    def shift_cells(self, c):
        c3 = self.chunk3(c)
        out = []
        for a in range(3):
            data_lo = self.lo[a] + c3[a] * self.chunk_size - self.band if self.grid[a] > 1 else self.lo[a]
            corner = int(math.floor(math.floor(data_lo / self.w0) / self.align)) * self.align
            out.append(((c3[a] - self.half[a]) << self.S) + self.low - corner)
        return out

    def shift(self, c):
        """T_c in model units, fp32 (the product of the integer voxel count and the voxel size, rounded once)."""
        return np.asarray([np.float32(t * self.w0) for t in self.shift_cells(c)], np.float32)

    def key_range(self, c):
        o = self.slot_origin(c)
        k = D._morton3(o[0] + (1 << 20), o[1] + (1 << 20), o[2] + (1 << 20))
        return k, k + (1 << (3 * self.S))



def halo_inner(voxel_size, adaptive_depth=1, dual_graph='lattice'):
    """How far INSIDE a neighbour's core a rank evaluates the blend (model units).  Lattice mesher: 2.5 finest voxels (the one-ring
    of halo cells and its refined lattice).  Adaptive dual graph: the hexahedra around a rank's own octree corners reach one leaf
    across the seam and the MISE split of that leaf looks one more leaf out -- leaves up to 2^(A-1) voxels wide, the rings of
    the finer MISE rounds half as deep each: 3 * 2^(A-1) + 1 voxels cover any mise_iter."""
    if dual_graph != 'adaptive':
        return 2.5 * voxel_size
    return (3.0 * (1 << (max(1, int(adaptive_depth)) - 1)) + 1.0) * voxel_size


def exchange_band(core, cidx3, grid, ov, w0, inner=None):
    """Where OTHER ranks evaluate this chunk's field: along every split axis with a neighbouring chunk, from
    ``inner`` (default 2.5 finest voxels: their one-ring of halo cells and its refined lattice; halo_inner) inside the shared
    face to ``ov`` outside it (the end of the blend weight).  Returns [(axis, lo, hi), ...]; see pack_field(band=)."""
    clo, chi = core
    inner = 2.5 * w0 if inner is None else float(inner)
    out = []
    for a in range(3):
        if grid[a] <= 1:
            continue
        if cidx3[a] > 0:
            out.append((a, clo[a] - ov, clo[a] + inner))
        if cidx3[a] < grid[a] - 1:
            out.append((a, chi[a] - inner, chi[a] + ov))
    return out


def halo_destinations(cores, margin, grid, owner, counts, world_size):
    """{chunk: [ranks that need its halo and do not own it]} -- pure geometry (cores, owners, which chunks hold points), so every
    rank computes the same table and a halo is sent only where it is read."""
    nonempty = [c for c in range(len(owner)) if counts[c] > 0]
    dest_of = {}
    for r in range(world_size):
        owned_r = [c for c in nonempty if owner[c] == r]
        for c in needed_chunks(cores, margin, grid, owned_r, nonempty):
            if owner[c] != r:
                dest_of.setdefault(c, []).append(r)
    return dest_of


def needed_chunks(cores, margin, grid, owned, candidates):
    """Chunks whose core grown by ``margin`` touches the core of an owned chunk (owned included)."""
    out = set(owned)
    for c in candidates:
        if c in out:
            continue
        clo, chi = cores[c]
        for o in owned:
            olo, ohi = cores[o]
            if all(grid[a] == 1 or (clo[a] - margin < ohi[a] and chi[a] + margin > olo[a]) for a in range(3)):
                out.add(c)
                break
    return sorted(out)


def chunk_grid_struct(origin, grid, chunk_size, sel_band, w_band, device, shift=None):
    """nksr_chunk_grid_t (include/nksr_hip.h) + the device arrays it points to (keep both alive).  Bounds are rounded to fp32 once,
    on the host: lo_sel/hi_sel = core -+ sel_band (membership of the solve), lo_w/hi_w = core -+ w_band (blend ramps)."""
    G = ChunkGridT()
    keep = []
    # candidate window of a point: its home chunk +- reach.  floor + 1, not ceil: the kernel finds the home chunk with x * (1 / chunk_size),
    # the host bounds with origin + j * chunk_size -- at an exact chunk boundary the two may differ by one
    reach = 1
    for b in (sel_band, w_band):
        if b is not None:
            reach = max(reach, int(math.floor(b / chunk_size)) + 1)
    if reach > 4:
        raise RuntimeError('chunk_size %g is too small for this hierarchy: a chunk is solved on its core + a band of %g (overlap + 1.5 coarsest '
                           'voxels), which must stay below 4 chunk sizes -- use chunk_size >= %g' % (chunk_size, max(b for b in (sel_band, w_band) if b is not None),
                                                                                              max(b for b in (sel_band, w_band) if b is not None) / 3.9))
    for a in range(3):
        G.grid[a] = int(grid[a])
        G.origin[a] = float(origin[a])
        if grid[a] <= 1:
            continue
        for band, lo_name, hi_name in ((sel_band, 'lo_sel', 'hi_sel'), (w_band, 'lo_w', 'hi_w')):
            if band is None:
                continue
            lo_t = torch.tensor([np.float32(origin[a] + j * chunk_size - band) for j in range(grid[a])], dtype=torch.float32, device=device)
            hi_t = torch.tensor([np.float32(origin[a] + j * chunk_size + chunk_size + band) for j in range(grid[a])], dtype=torch.float32, device=device)
            keep += [lo_t, hi_t]
            getattr(G, lo_name)[a] = ptr(lo_t)
            getattr(G, hi_name)[a] = ptr(hi_t)
    G.reach = reach
    G.inv_cs = float(np.float32(1.0) / np.float32(chunk_size))
    if w_band is not None:
        G.inv_2ov = float(np.float32(1.0) / np.float32(2 * w_band))
    if shift is not None:
        keep.append(shift)
        G.shift = ptr(shift)
    return G, keep


def chunk_pairs(G, mode, xyz, flag, weights):
    """The (point, chunk) pairs of csrc/chunks.hip: count per point, exclusive scan, fill.  ``mode`` 0: membership of the solve
    (core +- the struct's sel band), 1: positive blend weight (core +- ov); ``flag`` int32 per chunk, < 0 = chunk absent.  Returns
    (offsets [n + 1] int32, point index int64, chunk int32, weight, translated position) -- the pairs of a point in ASCENDING chunk
    order; the last two only when ``weights``, else None."""
    n = xyz.shape[0]
    dev = xyz.device
    counts = torch.empty(n + 1, dtype=torch.int32, device=dev)
    counts[n:] = 0
    call('nksr_chunk_pair_counts', C.byref(G), mode, ptr(xyz), n, ptr(flag), ptr(counts), stream())
    offs = ops.exclusive_sum_i32(counts)
    m = int(offs[n].item())
    index = torch.empty(m, dtype=torch.int64, device=dev)
    chunk = torch.empty(m, dtype=torch.int32, device=dev)
    w = torch.empty(m, dtype=torch.float32, device=dev) if weights else None
    xq = torch.empty((m, 3), dtype=torch.float32, device=dev) if weights else None
    if m:
        call('nksr_chunk_pair_fill', C.byref(G), mode, ptr(xyz), n, ptr(flag), ptr(offs), ptr(index), ptr(chunk), ptr(w) if weights else None,
             ptr(xq) if weights else None, stream())
    return offs, index, chunk, w, xq
