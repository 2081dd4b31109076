"""``sdf_from_points``: signed distance of query points to an oriented point cloud, from each query's k nearest reference
points (reference: ext/sdfgen/sdf_from_points.cu:142-235, bound in ext/sdfgen/bind.cpp:10-15; call sites models/loss.py:85
``sdf_from_points(query_pos, ref_xyz, ref_normal, 8, 0.02, False)[0]`` and dataset/av_gt_geometry.py:64-76
``nb_points=8, stdv=3.0, adaptive_knn=8``).

The reference builds a CUDA kd-tree (tinyflann), writes the k indices of every query and runs one of two kernels over them.
Here (nb_points <= 32): the reference cloud is binned once into a uniform grid (Morton sort + cell hash, ``neighbours.PointGrid``), an
octree is stacked on it (``neighbours.PointPyramid``: the same sorted points, cells x2 per level), and ONE kernel per call
(csrc/knn_sdf.hip ``k_sdf_pyramid``) takes every query to the scale at which the cloud is within one cell of it, keeps its k nearest
candidates sorted in registers while it descends the cells around it with box pruning, and evaluates the estimator from them -- no
index lists, no second pass.  What is left (queries farther from the cloud than 4 cells of the coarsest level; nb_points > 32,
which bisects for the k-th distance instead) goes through single grids 4x coarser per round (``neighbours.search_every_scale``: the
same kernel on one-level octrees; plain grids for the bisection), so every query gets an answer like with a kd-tree.  Measurement
knobs (tests/sdfgen_vs_ref.py --variants): ``NKSR_SDFGEN_SEARCH=rounds`` builds no octree and keeps everything on that path -- for
nb_points <= 32 that now means one-level octrees throughout --, ``NKSR_SDFGEN_LEAF`` / ``NKSR_SDFGEN_RINGS`` set the octree's scan
threshold (48) and the rings searched per level (4).
"""
import os

import torch

from ..neighbours import MAX_K, _RINGS, PointGrid, PointPyramid, _grid_args, choose_cell_size, search_every_scale
from .._lib import call, ptr, stream


def _use_pyramid(k):
    return 0 < k <= MAX_K and os.environ.get('NKSR_SDFGEN_SEARCH', 'pyramid') != 'rounds'


def _pyramid_knobs():
    return int(os.environ.get('NKSR_SDFGEN_LEAF', '0')), int(os.environ.get('NKSR_SDFGEN_RINGS', '4'))


def _mean_knn_distance(ref_xyz, k, cell, pyramid=None):
    """Per reference point (original order): mean distance to its k nearest reference points, itself included."""
    n, dev = ref_xyz.shape[0], ref_xyz.device
    out = torch.zeros(n, dtype=torch.float32, device=dev)
    rings = _pyramid_knobs()[1]

    def run(index, rows):               # the kernels answer EVERY point, in the grid's order: the rows asked for are kept
        std = torch.empty(n, dtype=torch.float32, device=dev)
        valid = torch.empty(n, dtype=torch.int32, device=dev)
        if isinstance(index, PointPyramid):
            pg = index.pg
            call('nksr_knn_mean_dist_pyramid', index.struct, n, int(k), rings if index is pyramid else _RINGS, ptr(std), ptr(valid), stream())
        else:
            pg = index
            call('nksr_knn_mean_dist', ptr(pg.xyz), n, *_grid_args(pg), int(k), _RINGS, ptr(std), ptr(valid), stream())
        ok = torch.empty(n, dtype=torch.bool, device=dev)
        ok[pg.perm] = valid > 0
        if rows is None:
            out[pg.perm] = std
            return ok
        back = torch.empty_like(std)
        back[pg.perm] = std
        sel = rows[ok[rows]]
        out[sel] = back[sel]
        return ok[rows]

    search_every_scale(ref_xyz, pyramid if _use_pyramid(k) else None, run, k, n, cell,
                       'sdf_from_points: %%d reference points found no %d neighbours' % k)
    return out


def sdf_from_points(queries, ref_xyz, ref_normal, nb_points, stdv, compute_grad=False, imls=False, adaptive_knn=0):
    """-> [sdf [Q]] or [sdf [Q], grad [Q, 3]] (float32), the reference's return convention."""
    if not (queries.is_cuda and ref_xyz.is_cuda and ref_normal.is_cuda):
        raise RuntimeError('sdf_from_points: GPU tensors required (MI355X-only)')
    k = int(nb_points)
    n = ref_xyz.shape[0]
    if n < max(k, int(adaptive_knn), 1):
        raise RuntimeError('sdf_from_points: %d reference points for nb_points=%d' % (n, k))
    dev = queries.device
    if not bool(torch.isfinite(queries).all() & torch.isfinite(ref_xyz).all() & torch.isfinite(ref_normal).all()):      # (one readback)
        raise RuntimeError('sdf_from_points: non-finite input')
    q = queries.to(torch.float32).contiguous()
    ref = ref_xyz.to(torch.float32).contiguous()
    nrm = ref_normal.to(torch.float32).contiguous()
    cell = choose_cell_size(ref, max(k, int(adaptive_knn), 8))
    leaf, rings = _pyramid_knobs()
    pyramid = None
    if _use_pyramid(k) or _use_pyramid(int(adaptive_knn)):
        pyramid = PointPyramid(PointGrid(ref, cell), leaf=leaf)
    ref_std = _mean_knn_distance(ref, int(adaptive_knn), cell, pyramid) if int(adaptive_knn) > 0 else None
    nq = q.shape[0]
    sdf = torch.zeros(nq, dtype=torch.float32, device=dev)
    grad = torch.zeros((nq, 3), dtype=torch.float32, device=dev) if compute_grad else None

    def run(index, rows):
        pg = index.pg if isinstance(index, PointPyramid) else index
        ns = nrm[pg.perm].contiguous()
        stds = ref_std[pg.perm].contiguous() if ref_std is not None else None
        if rows is None:                # every query: straight into the outputs
            qs, s, g = q, sdf, grad
        else:
            qs = q[rows].contiguous()
            s = torch.empty(qs.shape[0], dtype=torch.float32, device=dev)
            g = torch.empty((qs.shape[0], 3), dtype=torch.float32, device=dev) if compute_grad else None
        m = qs.shape[0]
        valid = torch.empty(m, dtype=torch.int32, device=dev)
        tail = (float(stdv), int(bool(imls)), ptr(s), ptr(g), ptr(valid), stream())
        if pg is index:
            call('nksr_sdf_from_points', ptr(pg.xyz), ptr(ns), ptr(stds), *_grid_args(pg), ptr(qs), m, k, _RINGS, *tail)
        else:
            call('nksr_sdf_from_points_pyramid', index.struct, ptr(ns), ptr(stds), ptr(qs), m, k, rings if index is pyramid else _RINGS, *tail)
        ok = valid > 0
        if rows is not None:
            sdf[rows[ok]] = s[ok]
            if compute_grad:
                grad[rows[ok]] = g[ok]
        return ok

    search_every_scale(ref, pyramid if _use_pyramid(k) else None, run, k, nq, cell, 'sdf_from_points: %%d queries found no %d neighbours' % k)
    return [sdf, grad] if compute_grad else [sdf]
