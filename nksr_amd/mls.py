"""Moving-least-squares projection of a point cloud on the GPU (surfaced as ``nksr.cloud.mls_project`` and ``smooth_mls``; the step is
PCL's ``MovingLeastSquares`` and CGAL's jet smoothing).

What moves a point: every query is replaced by its projection onto a low-order polynomial fitted to its neighbours within ``radius``
with Gaussian weights (csrc/mls.hip states the definition in full).  The same fit gives a normal that is smoother than kNN-PCA -- the
gradient of the fit, not a plane's normal --, mean and Gaussian curvature (positive mean curvature on a sphere with outward normals,
``MeshGeometry.mean_curvature``'s convention) and the surface variation l0 / (l0 + l1 + l2).  Queries need not be points of the cloud:
projecting arbitrary points onto the fitted surface resamples it.

  * ``mls_project`` / ``CloudIndex.mls_project``: one launch of ``k_mls_project`` on the grid of ``CloudIndex.radius_count(radius)`` ->
    ``MlsResult``.  ``order=1``: the weighted least-squares plane; ``order=2``: a quadric over it.  ``order_used`` says per row what was
    fitted: 0 = fewer than ``min_neighbors`` neighbours or collinear / coincident ones (the point comes back as it is, curvatures and
    variation NaN, the normal is the point's input normal where the queries are the cloud itself and normals were given, else NaN),
    1 = the plane (asked for, or the quadric's normal equations lost rank), 2 = the quadric.
  * ``smooth_mls``: ``iterations`` projections of the cloud onto its own surface, the index rebuilt on the moved points.
fp64 sums in a fixed order, no atomics: the same call gives the same bits.  GPU tensors only.
"""
import numpy as np
import torch

from . import cloud_input
from ._lib import call, ptr, require_gpu, stream

MIN_NEIGHBORS = {1: (3, 3), 2: (6, 8)}            # order -> (the floor: the unknowns of the fit, the default)


class MlsResult:
    """``position`` / ``normal`` float64 [Q, 3], ``mean_curvature`` / ``gaussian_curvature`` / ``variation`` float64 [Q] (NaN where not
    defined), ``count`` int32 [Q] = neighbours within the radius, ``order_used`` int8 [Q], ``valid`` bool [Q] = ``order_used > 0``;
    rows in the caller's order."""

    def __init__(self, position, normal, mean_curvature, gaussian_curvature, variation, count, order_used):
        self.position, self.normal, self.mean_curvature, self.gaussian_curvature = position, normal, mean_curvature, gaussian_curvature
        self.variation, self.count, self.order_used = variation, count, order_used
        self.valid = order_used > 0

    @property
    def xyz(self):
        """the positions rounded to float32"""
        return self.position.float()

    @property
    def normal32(self):
        """the normals rounded to float32"""
        return self.normal.float()

    def __repr__(self):
        return 'MlsResult(rows=%d, valid=%d)' % (self.count.numel(), int(self.valid.sum()))


def _check_args(what, radius, order, sigma, min_neighbors):
    """-> (radius as the fp32 value the kernel works with, sigma, order, min_neighbors); raises before anything touches a device"""
    radius = cloud_input.positive(radius, what, 'radius')
    if order not in (1, 2) or isinstance(order, bool):
        raise ValueError('%s: order must be 1 or 2 (got %r)' % (what, order))
    order = int(order)
    h = float(np.float32(radius))
    if not (0.0 < h < float('inf')):
        raise ValueError('%s: radius must be positive and finite in float32 (got %r)' % (what, radius))
    sigma = cloud_input.positive(0.5 * h if sigma is None else sigma, what, 'sigma')
    floor, default = MIN_NEIGHBORS[order]
    m = default if min_neighbors is None else int(min_neighbors)
    if m < floor:
        raise ValueError('%s: min_neighbors must be >= %d at order %d (got %r)' % (what, floor, order, min_neighbors))
    return h, sigma, order, m


def _check_normal(what, normal, n):
    """shape and type alone (ValueError): the device is compared once the index is there"""
    if normal is not None:
        cloud_input.rows_like(normal, n, None, what, 'normal', floating=True, error=ValueError)


def mls_on_index(index, radius, normal=None, query=None, order=2, sigma=None, min_neighbors=None):
    """``mls_project`` on a ``cloud.CloudIndex``.  A self-query runs in the Morton order of ``index._radius_grid(radius)`` (query NULL) and
    its rows are scattered back to the caller's order."""
    from .neighbours import _grid_args
    h, sigma, order, m = _check_args('mls_project', radius, order, sigma, min_neighbors)
    _check_normal('mls_project', normal, index.n)
    n, dev = index.n, index.device
    if n >= 1 << 31:
        raise ValueError('mls_project: %d points, at most 2^31 - 1' % n)
    g = index._radius_grid(float(radius))          # (the grid radius_count(radius) uses: cell = 1.02 radius >= fl32(radius))
    ns = None
    if normal is not None:
        cloud_input.rows_like(normal, n, dev, 'mls_project', 'normal')
        ns = g.to_grid(normal.to(torch.float32))
    if query is None:
        q, nq = None, n
    else:
        q = index._queries(query, g.cell)
        nq = q.shape[0]
    pos = torch.empty((nq, 3), dtype=torch.float64, device=dev)
    nrm = torch.empty((nq, 3), dtype=torch.float64, device=dev)
    mean, gauss, var = (torch.empty(nq, dtype=torch.float64, device=dev) for _ in range(3))
    count = torch.empty(nq, dtype=torch.int32, device=dev)
    used = torch.empty(nq, dtype=torch.int8, device=dev)
    call('nksr_mls_project', ptr(g.xyz), n, *_grid_args(g), ptr(ns), ptr(q), nq, h, sigma, order, m, ptr(pos), ptr(nrm), ptr(mean),
         ptr(gauss), ptr(var), ptr(count), ptr(used), stream())
    out = [pos, nrm, mean, gauss, var, count, used]
    if query is None:                       # grid order -> the caller's
        out = [g.to_caller(t) for t in out]
    return MlsResult(*out)


def mls_project(xyz, radius, normal=None, query=None, order=2, sigma=None, min_neighbors=None):
    """The moving-least-squares projection of ``query`` [Q, 3] (default: the cloud itself) onto the surface of the cloud ``xyz`` [N, 3],
    N >= 1 -> ``MlsResult``.  ``radius``: the neighbourhood (inclusive, decided in fp32 like ``CloudIndex.radius_count``); ``sigma``: the
    width of the Gaussian weights exp(-d^2 / sigma^2), default radius / 2; ``normal`` [N, 3]: signs the fitted normals (without it the
    largest component of a normal is made positive); ``min_neighbors``: default 3 (order 1) / 8 (order 2), never below 3 / 6."""
    from .cloud import CloudIndex
    _check_args('mls_project', radius, order, sigma, min_neighbors)
    cloud_input.rows3(xyz, 'mls_project')
    _check_normal('mls_project', normal, xyz.shape[0])
    return mls_on_index(CloudIndex(xyz), radius, normal, query, order, sigma, min_neighbors)


def smooth_mls(xyz, radius, normal=None, iterations=1, order=2, sigma=None, min_neighbors=None):
    """``iterations`` times: every point is projected onto the surface of the cloud as it then stands (``mls_project`` on an index
    rebuilt on the moved points; float32 between the iterations) -> (xyz' float32 [N, 3], normal' float32 [N, 3]).  A point with
    ``order_used == 0`` stays where it is and keeps its normal.  With ``normal`` the fitted normals are signed by it and replace it
    for the next iteration; without, every iteration signs its normals by their largest component and the last one's are returned
    (NaN rows where that iteration had ``order_used == 0``)."""
    _check_args('smooth_mls', radius, order, sigma, min_neighbors)
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 1:
        raise ValueError('smooth_mls: iterations must be an integer >= 1 (got %r)' % (iterations,))
    cloud_input.rows3(xyz, 'smooth_mls')
    _check_normal('smooth_mls', normal, xyz.shape[0])
    require_gpu(xyz.device)
    xyz = xyz.to(torch.float32)
    if normal is not None:
        normal = normal.to(torch.float32)
    if xyz.shape[0] == 0:
        return xyz, normal if normal is not None else xyz.clone()
    out_normal = normal
    for _ in range(int(iterations)):
        r = mls_project(xyz, radius, normal=normal, order=order, sigma=sigma, min_neighbors=min_neighbors)
        keep = r.valid[:, None]
        xyz = torch.where(keep, r.xyz, xyz)
        if normal is not None:
            normal = torch.where(keep, r.normal32, normal)
            out_normal = normal
        else:
            out_normal = r.normal32
    return xyz, out_normal
