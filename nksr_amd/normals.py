"""kNN-PCA normal estimation + sensor orientation on the GPU (csrc/knn_normals.hip).

Mirrors the recipe the reference ships in source form (examples/recons_waymo_cpu.py:21-41, the
stand-in for ``nksr.get_estimate_normal_preprocess_fn(64, 85.0)``, examples/recons_waymo.py:36):
  1. unoriented normals = smallest PCA eigenvector of the k nearest neighbours (k includes the
     point itself)
  2. flip so that the normal faces the sensor:  (sensor - xyz) . n >= 0
  3. drop grazing points: keep |cos| > cos(deg)
"""
import math

import torch

from ._lib import call, ptr, stream
from .neighbours import PointGrid, choose_cell_size


class TooFewPoints(RuntimeError):
    """Fewer points than the neighbourhood size: chunk mode treats such a chunk as empty (nksr_amd/chunking/driver.py)."""


def knn_pca(xyz, knn):
    """Unoriented kNN-PCA normals: (PointGrid, normal [n,3], r2 [n], valid [n]) in the grid's Morton order (``pg.perm`` maps back).
    ``r2`` is the squared distance of the k-th nearest neighbour (the point itself included): the neighbour SET of point i is
    {j : |x_i - x_j|^2 <= r2_i} -- the kernel keeps no index lists, this is what the parity test compares with an exact kd-tree."""
    n = xyz.shape[0]
    pg = PointGrid(xyz, choose_cell_size(xyz, knn))
    nrm = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    r2 = torch.empty(n, dtype=torch.float32, device=xyz.device)
    valid = torch.empty(n, dtype=torch.int32, device=xyz.device)
    todo = torch.empty(n, dtype=torch.int32, device=xyz.device)       # one wavefront per query; the queries it hands back (too many candidates)
    h = pg.grid.hash
    call('nksr_knn_pca_normals', ptr(pg.xyz), n, ptr(pg.start), ptr(pg.end), ptr(h.hkeys), ptr(h.hvals), h.cap, pg.cell,
         pg.inv_cell, int(knn), 6, ptr(nrm), ptr(r2), ptr(valid), ptr(todo), stream())
    return pg, nrm, r2, valid


def estimate_normals_knn(xyz, normal, sensor, knn=64, deg=85.0):
    """(xyz, normal=None, sensor) -> (xyz', normal', None), the preprocess_fn contract of
    examples/recons_waymo_cpu.py:21-41."""
    if normal is not None:
        raise RuntimeError('normal already exists')
    if sensor is None:
        raise RuntimeError('please provide sensor positions for consistent orientations')
    n = xyz.shape[0]
    if n < knn:
        raise TooFewPoints('need at least knn=%d points' % knn)
    pg, nrm, r2, valid = knn_pca(xyz, knn)
    xs = pg.xyz
    ss = sensor.to(torch.float32)[pg.perm]
    view = ss - xs
    view = view / (torch.linalg.norm(view, dim=-1, keepdim=True) + 1e-6)
    cos = (view * nrm).sum(1)
    nrm = torch.where((cos < 0)[:, None], -nrm, nrm)
    keep = (cos.abs() > math.cos(math.radians(deg))) & (valid > 0)
    # return in the original point order (stable w.r.t. the input, like the CPU recipe)
    order = torch.argsort(pg.perm[keep])
    return xs[keep][order].contiguous(), nrm[keep][order].contiguous(), None
