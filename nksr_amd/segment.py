"""Point-cloud segmentation on the GPU (surfaced as ``nksr.cloud.cluster_dbscan``, ``segment_plane`` and friends; names follow Open3D).

What a scan of a scene needs before ``Reconstructor.reconstruct`` sees it: the dominant plane (ground, floor, table) found and taken
out, and what is left split into its objects, so that small dense blobs and stray returns are dropped before they cost voxels.

  * ``cluster_dbscan`` / ``CloudIndex.cluster_dbscan``: density-based clusters.  The definition (csrc/segment.hip states it in
    full): j is a neighbour of i iff knn_d2(x_j - x_i) <= fl32(eps)^2 in fp32, inclusive, a point its own neighbour; core = at least
    ``min_points`` neighbours (``nksr_radius_count`` as it is); clusters = connected components of the core-core neighbour graph
    (``k_dbscan_hook``: union-find in the grid's Morton order); a non-core point takes the lowest label among its core neighbours
    (``k_dbscan_border``) or is noise (-1); labels ascend with the smallest caller index among each cluster's core points.  Integers
    only.  Sizes and centroids: ``cloud.voxel_reduce`` over the points sorted by label (fp64 sums in a fixed order).
  * ``segment_plane``: RANSAC.  Hypotheses from point triples on the host (``sample_planes``: one gather of 3 H points read back),
    scored in one launch (``plane_scores``: ``k_hypothesis_score`` of csrc/score_dev.h, integer counts), the best refined by the
    principal axes of its inliers (``k_plane_moments`` + ``nksr_icp_reduce``: fp64 sums in a fixed order; covariance and
    ``numpy.linalg.eigh`` on the host).
No floating-point atomics anywhere: the same call gives the same bits.  GPU tensors only.
"""
import numpy as np
import torch

from . import _lib, cloud_input, ops
from ._lib import call, ptr, stream

FIELDS = _lib.ICP_FIELDS
P_COUNT, P_SUM, P_MOMENT = _lib.PLANE_COUNT, _lib.PLANE_SUM, _lib.PLANE_MOMENT
MAX_POINTS = (1 << 31) - 1          # what the plane kernels index
DEGENERATE_NORMAL = 1e-12           # a triple whose (p1 - p0) x (p2 - p0) is no longer than this gives no plane


# ---- A. DBSCAN -------------------------------------------------------------------------------------------------------------------------
class DbscanResult:
    """``labels`` int64 [N] (-1 = noise), ``core`` bool [N], ``n_clusters``, ``sizes`` int64 [C] = points per cluster (core + border),
    ``centroid`` float32 [C, 3] = the mean of every cluster's points (fp64 sums in a fixed order, rounded once)."""

    def __init__(self, labels, core, n_clusters, sizes, centroid):
        self.labels, self.core, self.n_clusters, self.sizes, self.centroid = labels, core, n_clusters, sizes, centroid

    def __repr__(self):
        return 'DbscanResult(n_clusters=%d, noise=%d of %d)' % (self.n_clusters, int((self.labels < 0).sum()), self.labels.numel())

    def select(self, min_cluster_size=None, keep_largest=None):
        """bool [C]: clusters with at least ``min_cluster_size`` points; with ``keep_largest=k`` only the k largest of those (ties on
        size go to the lower label)."""
        keep = torch.ones(self.n_clusters, dtype=torch.bool, device=self.sizes.device)
        if min_cluster_size is not None:
            keep &= self.sizes >= int(min_cluster_size)
        if keep_largest is not None and self.n_clusters:
            if int(keep_largest) < 0:
                raise ValueError('select: keep_largest must be >= 0 (got %r)' % (keep_largest,))
            size = torch.where(keep, self.sizes, torch.full_like(self.sizes, -1))
            top = torch.zeros_like(keep)
            top[torch.sort(size, descending=True, stable=True)[1][:int(keep_largest)]] = True       # (stable: the lower label first)
            keep &= top
        return keep

    def point_mask(self, keep):
        """bool [N]: the points of the clusters flagged in ``keep`` [C]; noise: False."""
        if self.n_clusters == 0:
            return torch.zeros_like(self.core)
        return keep[self.labels.clamp(min=0)] & (self.labels >= 0)


def _check_dbscan(eps, min_points):
    eps, m = cloud_input.positive(eps, 'cluster_dbscan', 'eps'), int(min_points)
    if m < 1:
        raise ValueError('cluster_dbscan: min_points must be >= 1 (got %r)' % (min_points,))
    return eps, m


def _empty_result(dev):
    return DbscanResult(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.bool, device=dev), 0,
                        torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev))


def cluster_stats(xyz, labels, n_clusters):
    """(sizes int64 [C], centroid float32 [C, 3]): the non-noise points sorted by label (stable: ascending index inside a cluster), one
    run per label, reduced by ``cloud.voxel_reduce``."""
    from .cloud import voxel_reduce
    dev = xyz.device
    if n_clusters == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev)
    member = torch.nonzero(labels >= 0).flatten()
    sorted_labels, order = ops.sort_pairs(labels[member], member.to(torch.int32), end_bit=ops._bits(n_clusters))
    nr, start, _, _ = ops.sorted_runs(sorted_labels)
    assert nr == n_clusters                          # (every cluster holds a core point)
    mean, _, count, _ = voxel_reduce(order, start[:-1], start[1:], xyz)
    return count.long(), mean


def dbscan_on_index(index, eps, min_points):
    """``cluster_dbscan`` on a ``cloud.CloudIndex``: everything up to the labels runs in the Morton order of
    ``index._radius_grid(eps)`` and is scattered back to the caller's order at the end.  Syncs twice (the number of clusters, the runs)."""
    from .neighbours import _grid_args
    eps, m = _check_dbscan(eps, min_points)
    n, dev = index.n, index.device
    if n >= 1 << 31:
        raise ValueError('cluster_dbscan: %d points, at most 2^31 - 1' % n)
    g = index._radius_grid(eps)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_radius_count', ptr(g.xyz), n, *_grid_args(g), None, n, eps, m, 0, None, ptr(count), stream())
    core = (count >= m).to(torch.uint8)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n + 1, dtype=torch.int32, device=dev)
    call('nksr_dbscan_components', ptr(g.xyz), n, *_grid_args(g), eps, ptr(core), ptr(parent), ptr(flags), stream())
    # label order: the roots (minimum SORTED indices) ranked by the minimum CALLER index of their component
    first = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_dbscan_min_caller', ptr(parent), ptr(g.perm), n, ptr(first), stream())
    roots = torch.nonzero(flags[:n]).flatten()
    nc = int(roots.numel())
    _, by_first = ops.sort_pairs(first[roots].long(), roots.to(torch.int32), end_bit=ops._bits(n))
    rank = torch.zeros(n, dtype=torch.int32, device=dev)
    rank[by_first.long()] = torch.arange(nc, dtype=torch.int32, device=dev)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_uf_labels', ptr(parent), n, ptr(rank), ptr(label), stream())
    call('nksr_dbscan_border', ptr(g.xyz), n, *_grid_args(g), eps, ptr(core), ptr(label), stream())
    labels, core_out = g.to_caller(label.long()), g.to_caller(core.bool())
    sizes, centroid = cluster_stats(index.xyz, labels, nc)
    return DbscanResult(labels, core_out, nc, sizes, centroid)


def cluster_dbscan(xyz, eps, min_points):
    """Density-based clusters of ``xyz`` [N, 3] (Open3D's ``cluster_dbscan``; the definition: this module's docstring) ->
    ``DbscanResult``.  ``min_points=1`` makes every point core; an empty cloud gives empty results."""
    from .cloud import CloudIndex, _amax
    _check_dbscan(eps, min_points)
    _amax(xyz)
    if xyz.shape[0] == 0:
        return _empty_result(xyz.device)
    return dbscan_on_index(CloudIndex(xyz), eps, min_points)


# ---- B. plane RANSAC -------------------------------------------------------------------------------------------------------------------
def _check_threshold(t, what):
    t = float(t)
    if not (0.0 <= t < float('inf')):
        raise ValueError('%s: distance_threshold must be finite and not negative (got %r)' % (what, t))
    return t


def sample_planes(xyz, num_iterations, seed=0):
    """The RANSAC hypotheses: -> (planes float64 numpy [H, 4], triples int64 numpy [H, 3]).  Triples are
    ``numpy.random.RandomState(seed).randint(0, N, (H, 3))``; their 3 H points are gathered on the device and read back once; in fp64
    numpy n = (p1 - p0) x (p2 - p0), scaled to unit length, d = -n . p0.  A triple with |n| <= 1e-12 before scaling is degenerate: its
    row is all zeros, and it scores -1."""
    xyz = cloud_input.points(xyz, 'sample_planes', max_rows=MAX_POINTS)
    h, n = int(num_iterations), xyz.shape[0]
    if h < 1:
        raise ValueError('sample_planes: num_iterations must be >= 1 (got %r)' % (num_iterations,))
    if n < 1:
        raise ValueError('sample_planes: empty cloud')
    triples = np.random.RandomState(seed).randint(0, n, (h, 3)).astype(np.int64)
    p = xyz[torch.from_numpy(triples.reshape(-1)).to(xyz.device)].cpu().numpy().astype(np.float64).reshape(h, 3, 3)
    return planes_of_triples(p), triples


def planes_of_triples(p):
    """float64 [H, 3, 3] points -> float64 [H, 4] planes (zeros where degenerate)."""
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.sqrt((normal * normal).sum(1))
    ok = length > DEGENERATE_NORMAL
    unit = normal / np.where(ok, length, 1.0)[:, None]
    planes = np.concatenate([unit, -(unit * p[:, 0]).sum(1, keepdims=True)], axis=1)
    planes[~ok] = 0.0
    return planes


def plane_scores(xyz, planes, distance_threshold):
    """int32 [H] on the device: the number of points of ``xyz`` with |((a x + b y) + c z) + d| <= ``distance_threshold`` (fp64, no
    fused multiply-add) for every row (a, b, c, d) of ``planes`` (float64 [H, 4], numpy or tensor); -1 for a degenerate row."""
    xyz = cloud_input.points(xyz, 'plane_scores', max_rows=MAX_POINTS)
    t = _check_threshold(distance_threshold, 'plane_scores')
    pl = torch.as_tensor(planes, dtype=torch.float64)
    if pl.dim() != 2 or pl.shape[1] != 4:
        raise ValueError('plane_scores: planes must be [H, 4] (got shape %s)' % (tuple(pl.shape),))
    pl = pl.to(xyz.device).contiguous()
    counts = torch.empty(pl.shape[0], dtype=torch.int32, device=xyz.device)
    call('nksr_plane_score', ptr(xyz), xyz.shape[0], ptr(pl), pl.shape[0], t, ptr(counts), stream())
    return counts


def sign_normal(plane):
    """the plane with its sign fixed: the first non-zero of (n_z, n_y, n_x) is positive"""
    for a in (2, 1, 0):
        if plane[a] != 0.0:
            return plane if plane[a] > 0.0 else -plane
    return plane


def plane_from_moments(sums, centre):
    """The least-squares plane of the inliers from their sums about ``centre`` (float64 [NKSR_ICP_FIELDS], layout: include/nksr_hip.h):
    covariance, ``numpy.linalg.eigh``, the eigenvector of the smallest eigenvalue, signed by ``sign_normal``, d = -n . mean.  None
    with fewer than 3 inliers."""
    sums, centre = np.asarray(sums, np.float64), np.asarray(centre, np.float64)
    n = sums[P_COUNT]
    if not n >= 3:
        return None
    m = sums[P_SUM:P_SUM + 3] / n
    S = np.zeros((3, 3))
    S[np.triu_indices(3)] = sums[P_MOMENT:P_MOMENT + 6]
    S = S + np.triu(S, 1).T
    cov = S / n - np.outer(m, m)
    _, vec = np.linalg.eigh(cov)
    normal = vec[:, 0]
    return sign_normal(np.concatenate([normal, [-normal @ (centre + m)]]))


class PlanePass:
    """``run(plane)`` -> (mask uint8 [N] on the device, sums float64 numpy [NKSR_ICP_FIELDS]: one 256-byte read) for one cloud."""

    def __init__(self, xyz, threshold):
        from .register import RowSums
        self.xyz, self.t, self.n = xyz, threshold, xyz.shape[0]
        self.centre = cloud_input.bbox_centre64(xyz)
        self.rows = RowSums(self.n, 4, xyz.device)                            # the plane's 4

    def run(self, plane):
        rows = self.rows
        rows.set(plane, self.centre)
        mask = torch.empty(self.n, dtype=torch.uint8, device=self.xyz.device)
        call('nksr_plane_moments', ptr(self.xyz), self.n, rows.args_ptr, rows.centre_ptr, self.t, ptr(mask), ptr(rows.partials), stream())
        return mask, rows.reduce()


def segment_plane(xyz, distance_threshold, ransac_n=3, num_iterations=1000, seed=0):
    """The dominant plane of ``xyz`` [N, 3] (Open3D's ``segment_plane``) -> (plane float64 numpy [4] = (a, b, c, d) with |(a, b, c)| = 1,
    inliers int64 [M] on the device, ascending).  ``num_iterations`` hypotheses (``sample_planes``) are scored (``plane_scores``); the
    best is the highest count, the lowest iteration on a tie.  It is refined once: the least-squares plane of its inliers
    (``plane_from_moments``; kept as it is with fewer than 3 of them).  The inliers returned are the points within
    ``distance_threshold`` of the REFINED plane."""
    if int(ransac_n) != 3:
        raise ValueError('segment_plane: ransac_n must be 3 (got %r)' % (ransac_n,))
    xyz = cloud_input.points(xyz, 'segment_plane', max_rows=MAX_POINTS)
    t = _check_threshold(distance_threshold, 'segment_plane')
    if xyz.shape[0] < 3:
        raise ValueError('segment_plane: a plane needs at least 3 points (got %d)' % xyz.shape[0])
    cloud_input.all_finite(xyz, 'segment_plane')
    planes, _ = sample_planes(xyz, num_iterations, seed)
    counts = plane_scores(xyz, planes, t).cpu().numpy()
    best = int(np.argmax(counts))                       # (the first of the maxima: the lowest iteration)
    if counts[best] < 0:
        raise RuntimeError('segment_plane: every one of the %d sampled triples is degenerate (collinear or repeated points)' % len(counts))
    ps = PlanePass(xyz, t)
    plane = planes[best]
    _, sums = ps.run(plane)
    refined = plane_from_moments(sums, ps.centre)
    if refined is not None and np.all(np.isfinite(refined)):
        plane = refined
    mask, _ = ps.run(plane)
    return plane.copy(), torch.nonzero(mask).flatten()
