"""Neighbour search over a point cloud (csrc/knn_dev.h, knn_walk_dev.h, knn_topk_dev.h and the kernels on them: knn_normals.hip, knn_sdf.hip,
knn_query.hip, metrics.hip): the Morton grid, the octree stacked on it, the cell size that suits a
neighbourhood size, and the one loop that takes a search through every scale.  Used by the normals, ``ext.sdfgen``, the mesh metrics,
``cloud.CloudIndex`` and the colour field.
"""
import math

import torch

from . import ops
from ._lib import KNN_LEVELS, KnnPyramidT, call, ptr, stream
from .svh import SparseGrid, inv_w0_f32

MAX_K = 32              # csrc/knn_topk_dev.h keeps the candidates of k <= 32 sorted in registers; more neighbours take the bisection kernels
_RINGS = 4              # rings searched per grid when a search is retried on coarser cells
_MAX_ROUNDS = 16        # the cell size grows 4x per round: 4^16 cells of the first size span any finite cloud


class PointGrid:
    """Uniform grid over a cloud: Morton-sorted points + per-cell ranges + cell hash."""

    def __init__(self, xyz, cell):
        xyz = xyz.to(torch.float32).contiguous()
        n = xyz.shape[0]
        dev = xyz.device
        self.cell = float(cell)
        self.inv_cell = inv_w0_f32(cell)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        call('nksr_point_keys', ptr(xyz), n, self.inv_cell, ptr(keys), stream())
        ks, perm = ops.sort_pairs(keys, torch.arange(n, dtype=torch.int32, device=dev))
        self.perm = perm.long()
        self.xyz = xyz[self.perm].contiguous()
        self.keys_sorted = ks
        self.grid = SparseGrid(ops.unique_sorted(ks), 0, cell)
        self.start = torch.empty(self.grid.num_voxels, dtype=torch.int32, device=dev)
        self.end = torch.empty(self.grid.num_voxels, dtype=torch.int32, device=dev)
        call('nksr_site_ranges', ptr(ks), n, ptr(self.grid.keys), self.grid.num_voxels, 0, ptr(self.start), ptr(self.end), stream())

    def to_grid(self, t):
        """rows in the caller's order -> the grid's (Morton) order, contiguous"""
        return t[self.perm].contiguous()

    def to_caller(self, t):
        """rows in the grid's order -> the caller's, in a fresh tensor"""
        out = torch.empty_like(t)
        out[self.perm] = t
        return out

    def nearest(self, query, max_ring=8):
        """Index (into the ORIGINAL cloud order) of the nearest point of every query."""
        q = query.to(torch.float32).contiguous()
        idx = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        h = self.grid.hash
        call('nksr_nearest_index', ptr(self.xyz), ptr(self.start), ptr(self.end), ptr(h.hkeys), ptr(h.hvals), h.cap, self.cell,
             self.inv_cell, ptr(q), q.shape[0], int(max_ring), ptr(idx), stream())
        ok = idx >= 0
        out = torch.full_like(idx, -1, dtype=torch.int64)
        out[ok] = self.perm[idx[ok].long()]
        return out


class PointPyramid:
    """Octree over a ``PointGrid``: level l = cells of size cell * 2^l (keys = the grid's keys >> 3 l), each with its point range, the
    range of its children on the level below and their octant mask, and a key hash (csrc/knn_topk_dev.h ``KnnPyramid``).  Built upward from
    the grid until a level has <= ``top_cells`` cells (one kernel + one hash per level; the level sizes come back to the host) or
    there are ``max_levels`` of them -- ``max_levels=1``: the grid alone, as the search kernels take it.
    Eight, not one: keys are biased coordinates, so the cells either side of a coordinate plane through the origin never merge."""

    def __init__(self, pg, leaf=0, top_cells=8, max_levels=KNN_LEVELS):
        dev = pg.xyz.device
        self.pg = pg
        keys, start, end = pg.grid.keys, pg.start, pg.end
        self.keep = [keys, start, end]
        t = KnnPyramidT()
        t.xyz_sorted = ptr(pg.xyz)
        t.cell, t.inv_cell, t.leaf = pg.cell, pg.inv_cell, int(leaf)
        h = pg.grid.hash
        lvl = 0
        while True:
            t.start[lvl], t.end[lvl], t.hkeys[lvl], t.hvals[lvl], t.hcap[lvl] = ptr(start), ptr(end), ptr(h.hkeys), ptr(h.hvals), h.cap
            lvl += 1
            nc = keys.numel()
            if lvl == min(max_levels, KNN_LEVELS) or nc <= top_cells:
                break
            up = ops.unique_sorted(keys >> 3)
            n = up.numel()
            child = torch.empty(n + 1, dtype=torch.int32, device=dev)
            cmask = torch.empty(n, dtype=torch.uint8, device=dev)
            s2 = torch.empty(n, dtype=torch.int32, device=dev)
            e2 = torch.empty(n, dtype=torch.int32, device=dev)
            call('nksr_knn_pyramid_level', ptr(keys), nc, ptr(start), ptr(end), ptr(up), n, ptr(child), ptr(cmask), ptr(s2), ptr(e2), stream())
            h = ops.HashTable(up)
            t.child[lvl], t.cmask[lvl] = ptr(child), ptr(cmask)
            self.keep += [up, child, cmask, s2, e2, h]
            keys, start, end = up, s2, e2
        t.levels = lvl
        self.levels = lvl
        self.top_keys = keys                    # sorted keys of the top level (the exhaustive pass of nksr_nn_metrics)
        self.top_cell = pg.cell * (1 << (lvl - 1))
        self.struct = t


def choose_cell_size(xyz, k):
    """Cell size such that a ball of one cell radius holds ~2k surface samples: density from the
    occupied-voxel count at one probe resolution (points on a surface: count ~ area / cell^2)."""
    from .density import bbox_center, occupied_voxels
    n = xyz.shape[0]
    lo, hi, center = bbox_center(xyz)
    ext = float((hi - lo).max())
    # the probe voxels must hold several samples each or their count saturates at n and the density comes out as 1 / probe^2 whatever
    # the cloud (4 000 points at ext / 256: one point per cell, every kNN query ran to its outermost ring): a surface of area ~ ext^2
    # sampled n times has ~4 samples per voxel of size 4 ext / sqrt(n); from 1 M points on that is finer than ext / 256 and nothing changes
    probe = max(ext / 256.0, 4.0 * ext / math.sqrt(max(n, 1)), 1e-6)
    occ = max(occupied_voxels((xyz - lo[None]).contiguous(), probe), 1)
    area = occ * probe * probe                      # ~ surface area
    rho = n / max(area, 1e-20)
    return max(math.sqrt(2.0 * k / (math.pi * rho)), probe / 8)


def _grid_args(pg):
    h = pg.grid.hash
    return ptr(pg.start), ptr(pg.end), ptr(h.hkeys), ptr(h.hvals), h.cap, pg.cell, pg.inv_cell


def search_every_scale(ref, pyramid, run, k, n_rows, cell, failure):
    """Run a k-nearest-neighbour search until every one of ``n_rows`` rows has its answer.  ``run(index, rows)`` searches ``index``
    for the rows ``rows`` (int64 indices; None = all of them), stores what it finds and returns a bool mask over those rows: False =
    fewer than k points in reach on this scale.  First ``pyramid``, the octree over ``ref``, for all rows; what it hands back (rows
    farther from the cloud than ``_RINGS`` cells of its top level) goes to single grids, 4x coarser per round, so every row gets an
    answer like with a kd-tree: one-level ``PointPyramid``s for k <= ``MAX_K``, plain ``PointGrid``s (the bisection entry points)
    above.  ``pyramid=None``: single grids from the start, the first with cell ``cell``.  ``failure``: the message, with a %d for
    the number of rows, raised when rows remain after ``_MAX_ROUNDS`` rounds."""
    if pyramid is not None:
        rows = torch.nonzero(~run(pyramid, None)).flatten()
        cell = pyramid.top_cell * 2.0
    else:
        rows = torch.arange(n_rows, device=ref.device)
    for _ in range(_MAX_ROUNDS):
        if not rows.numel():
            return
        pg = PointGrid(ref, cell)
        rows = rows[~run(PointPyramid(pg, max_levels=1) if k <= MAX_K else pg, rows)]
        cell *= 4.0
    if rows.numel():
        raise RuntimeError(failure % rows.numel())
