"""Point-cloud preprocessing on the GPU: k-nearest-neighbour and radius queries, voxel downsampling, outlier masks.

The input side of the tool-chain (``MeshEvaluator`` / ``MeshQuery`` / ``MeshTopology`` are the output side): what a raw lidar or
photogrammetry scan needs before ``Reconstructor.reconstruct`` -- thinning to a working density and dropping stray returns -- and
the neighbour search the package already runs for its normals, its SDF ground truth and its metrics, with the indices handed out.

  * ``CloudIndex(xyz)``: the Morton grid and octree of csrc/knn_query.hip (``neighbours.PointGrid`` / ``PointPyramid``) built once;
    ``.knn`` / ``.radius_count`` / ``.mean_knn_distance`` (kernels ``k_knn_query_pyramid``, ``k_radius_count``).
  * ``voxel_downsample``: one point per occupied voxel, the mean (or the input point nearest the mean) of every attribute
    (csrc/cloud.hip ``k_voxel_reduce``: fp64 sums in a fixed order, no atomics, bitwise repeatable).
  * ``radius_outlier_mask`` / ``statistical_outlier_mask``.
  * ``orient_graph`` / ``orient_normals`` / ``estimate_normals`` (nksr_amd/orient.py, csrc/orient.hip): oriented normals for a cloud
    that has positions only -- signs propagated along the minimum spanning forest of the kNN graph.
  * ``icp`` / ``icp_multiscale`` / ``evaluate_registration`` / ``apply_transform`` / ``IcpResult`` (nksr_amd/register.py,
    csrc/register.hip): rigid registration of one cloud onto another, point-to-point or point-to-plane, before scans are merged.
  * ``cluster_dbscan`` / ``segment_plane`` / ``plane_scores`` / ``sample_planes`` / ``DbscanResult`` (nksr_amd/segment.py,
    csrc/segment.hip): a scene split into its objects -- density-based clusters, and the dominant plane found by RANSAC.
  * ``compute_fpfh_feature`` / ``match_features`` / ``registration_ransac_based_on_feature_matching`` / ``register_global`` /
    ``FpfhFeature`` / ``RansacResult`` (nksr_amd/global_register.py, csrc/fpfh.hip, csrc/global_register.hip): a pose for scans
    that share no frame -- FPFH features, matched by brute force, RANSAC over the matched pairs -- handed to ``icp``.
  * ``mls_project`` / ``smooth_mls`` / ``MlsResult`` (nksr_amd/mls.py, csrc/mls.hip): moving-least-squares projection -- the points
    moved onto a polynomial fitted to their neighbours (denoising, resampling), with the fit's normals, curvatures and variation.
``nksr_amd.preprocess`` wraps them as ``preprocess_fn`` for ``Reconstructor.reconstruct``.  GPU tensors only.
"""
import torch

from . import cloud_input, ops
from ._lib import call, ptr, require_gpu, stream
from .neighbours import MAX_K, _RINGS, PointGrid, PointPyramid, _grid_args, choose_cell_size, search_every_scale
from .orient import OrientedNormals, estimate_normals, orient_graph, orient_normals  # noqa: F401  (part of this module's surface)
from .register import IcpResult, apply_transform, evaluate_registration, icp, icp_multiscale  # noqa: F401  (part of this module's surface)
from .segment import DbscanResult, cluster_dbscan, plane_scores, sample_planes, segment_plane  # noqa: F401  (part of this module's surface)
from .global_register import (FpfhFeature, RansacResult, compute_fpfh_feature, match_features, register_global,  # noqa: F401  (part of this module's surface)
                              registration_ransac_based_on_feature_matching)
from .mls import MlsResult, mls_project, smooth_mls  # noqa: F401  (part of this module's surface)
from .svh import inv_w0_f32


def _check_points(xyz, cell, what='xyz'):
    """``cloud_input.points`` that a grid of ``cell`` can hold: finite, |x| / cell below 2^20 -- the checks of ``svh._check_xyz`` (one
    readback)."""
    xyz = cloud_input.points(xyz, None, what)
    if xyz.shape[0]:
        amax = float(xyz.abs().max())
        if not (amax * inv_w0_f32(cell) < (1 << 20) - 8):            # also catches NaN / inf
            raise RuntimeError('%s: coordinates non-finite or out of range: |x| / cell must stay below 2^20 (got %g); recentre the '
                               'cloud or use a larger cell' % (what, amax * inv_w0_f32(cell)))
    return xyz


def _amax(xyz):
    """max |x| of a cloud in the dtype it came in (the grid's cell is chosen from it), RuntimeError unless finite"""
    cloud_input.rows3(xyz, None)
    require_gpu(xyz.device)
    amax = float(xyz.abs().max()) if xyz.shape[0] else 0.0
    if not amax < float('inf'):
        raise RuntimeError('non-finite coordinates in the input')
    return amax


class CloudIndex:
    """Neighbour queries on one cloud.  ``xyz``: [N, 3] GPU tensor, N >= 1.  Indices that come back refer to the caller's order."""

    def __init__(self, xyz):
        amax = _amax(xyz)
        if xyz.shape[0] < 1:
            raise ValueError('CloudIndex: empty cloud')
        x32 = xyz.to(torch.float32).contiguous()
        # the cell of the normals / sdfgen searches (a few times 8 points per 3^3 block), kept wide enough for the cloud's coordinates
        # to stay inside the key range whatever its density (a single point, a thousand duplicates)
        cell = max(choose_cell_size(x32, 8), amax * 2.0 ** -15, 1e-9)
        self.xyz = _check_points(x32, cell)
        self.n = self.xyz.shape[0]
        self.device = self.xyz.device
        self.amax = amax
        self.pyramid = PointPyramid(PointGrid(self.xyz, cell))
        self.pg = self.pyramid.pg
        self._radius_grids = {}
        self._centre = None

    # ---- helpers -------------------------------------------------------------------------------------------------------------
    def _queries(self, query, cell):
        q = _check_points(query, cell, 'query')
        if q.device != self.device:
            raise RuntimeError('query is on %s, the cloud on %s' % (q.device, self.device))
        return q

    def _ranks(self, pg):
        """sorted position of every (caller-order) point in grid ``pg``"""
        return pg.to_caller(torch.arange(self.n, dtype=torch.int32, device=self.device))

    # ---- k nearest neighbours ------------------------------------------------------------------------------------------------
    def knn(self, k, query=None, exclude_self=False):
        """-> (idx int64 [Q, k], dist float32 [Q, k] ascending).  ``query=None``: the cloud itself, row i = point i.  ``exclude_self``
        (self-queries only): point i is left out of its own row; other points at the same position are not."""
        idx, d2 = self.knn_d2(k, query, exclude_self)
        return idx, torch.sqrt(d2)

    def knn_d2(self, k, query=None, exclude_self=False):
        """``knn`` with the SQUARED fp32 distances as the kernel wrote them (what the feature kernels are defined on)."""
        k = int(k)
        ex = bool(exclude_self)
        if k < 1 or k > MAX_K:
            raise ValueError('knn: 1 <= k <= %d (got %d)' % (MAX_K, k))
        if k + ex > self.n:
            raise ValueError('knn: k = %d%s of a cloud of %d points' % (k, ' other points' if ex else '', self.n))
        if ex and query is not None:
            raise ValueError('knn: exclude_self needs query=None (the cloud itself)')
        dev, pg = self.device, self.pg
        if query is None:
            q, nq = None, self.n
        else:
            q = self._queries(query, pg.cell)
            nq = q.shape[0]
        out_idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
        out_d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)

        def run(index, rows):
            g, full = index.pg, rows is None
            if full:                        # every row; a self-query runs in the grid's order (query NULL) and goes back to the caller's
                qs, me, m = q, None, nq
                rows = g.perm if query is None else slice(None)
            else:
                qs = (self.xyz if query is None else q)[rows].contiguous()
                me = self._ranks(g)[rows].contiguous() if ex else None
                m = rows.numel()
            idx = torch.zeros((m, k), dtype=torch.int32, device=dev)         # (zeroed: a row the search hands back is not written)
            d2 = torch.zeros((m, k), dtype=torch.float32, device=dev)
            valid = torch.empty(m, dtype=torch.int32, device=dev)
            call('nksr_knn_query_pyramid', index.struct, self.n, ptr(qs), m, k, int(ex), ptr(me), _RINGS, ptr(idx), ptr(d2), ptr(valid), stream())
            good = valid > 0
            if full:                        # all rows at once: written through, the rows handed back are overwritten later
                out_idx[rows] = g.perm[idx.long()]
                out_d2[rows] = d2
                ok = torch.empty_like(good)
                ok[rows] = good
                return ok
            out_idx[rows[good]] = g.perm[idx[good].long()]
            out_d2[rows[good]] = d2[good]
            return good

        search_every_scale(self.xyz, self.pyramid, run, k, nq, None, 'knn: %%d queries found no %d neighbours' % k)
        return out_idx, out_d2

    def mean_knn_distance(self, k):
        """float32 [N]: mean distance of every point to its k nearest OTHER points (the mean is taken in fp64 and rounded once)."""
        _, dist = self.knn(k, exclude_self=True)
        return dist.double().mean(dim=1).float()

    def orient_normals(self, normal, k=16, seed='+z', viewpoint=None):
        """``orient.orient_normals`` on this index: ``normal`` [N, 3] (any sign) oriented along the minimum spanning forest of
        ``knn(k, exclude_self=True)`` -> ``OrientedNormals``.  The kernels visit the points in the grid's Morton order."""
        from .orient import _orient_on_index
        return _orient_on_index(self, normal, k, seed, viewpoint)

    # ---- fixed-radius neighbour count ----------------------------------------------------------------------------------------
    def _radius_grid(self, radius):
        """A grid whose cell is >= radius: 2 % above it -- the fp32 product that bins a point is off by at most 2^-24 |x| / cell cells,
        < 2^-9 with the floor below -- and never so fine that the cloud's coordinates leave the key range."""
        if radius not in self._radius_grids:
            self._radius_grids.clear()                  # (one at a time: a grid is as large as the cloud)
            self._radius_grids[radius] = PointGrid(self.xyz, max(radius * 1.02, self.amax * 2.0 ** -15))
        return self._radius_grids[radius]

    def radius_count(self, radius, query=None, cap=None, exclude_self=False):
        """-> int32 [Q]: the number of cloud points within ``radius`` of every query (``query=None``: of every point of the cloud,
        itself counted unless ``exclude_self``).  ``cap``: counting stops there, the result is min(count, cap)."""
        radius = cloud_input.positive(radius, 'radius_count', 'radius')
        ex = bool(exclude_self)
        if ex and query is not None:
            raise ValueError('radius_count: exclude_self needs query=None (the cloud itself)')
        if cap is not None and int(cap) < 1:
            raise ValueError('radius_count: cap must be >= 1 (got %r)' % cap)
        g = self._radius_grid(radius)
        dev = self.device
        if query is None:
            q, nq = None, self.n
        else:
            q = self._queries(query, g.cell)
            nq = q.shape[0]
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        call('nksr_radius_count', ptr(g.xyz), self.n, *_grid_args(g), ptr(q), nq, radius, int(cap) if cap is not None else 0, int(ex), None,
             ptr(cnt), stream())
        return cnt if query is not None else g.to_caller(cnt)

    # ---- clusters --------------------------------------------------------------------------------------------------------------
    def cluster_dbscan(self, eps, min_points):
        """``segment.cluster_dbscan`` on this index (the grid of ``radius_count(eps)``) -> ``DbscanResult``."""
        from .segment import dbscan_on_index
        return dbscan_on_index(self, eps, min_points)

    # ---- moving least squares ------------------------------------------------------------------------------------------------
    def mls_project(self, radius, normal=None, query=None, order=2, sigma=None, min_neighbors=None):
        """``mls.mls_project`` on this index (the grid of ``radius_count(radius)``): ``query`` [Q, 3] (default: the cloud itself)
        projected onto the fitted surface -> ``MlsResult`` (rows in the caller's order)."""
        from .mls import mls_on_index
        return mls_on_index(self, radius, normal, query, order, sigma, min_neighbors)

    # ---- registration ----------------------------------------------------------------------------------------------------------
    def bbox_centre(self):
        """float64 numpy [3]: the centre of the cloud's bounding box (the point the registration sums are taken about)."""
        if self._centre is None:
            self._centre = cloud_input.bbox_centre64(self.xyz)
        return self._centre

    def compute_fpfh_feature(self, normal, radius, max_nn=32):
        """``global_register.compute_fpfh_feature`` on this index: ``normal`` [N, 3] -> ``FpfhFeature`` (rows in the caller's order)."""
        from .global_register import fpfh_on_index
        return fpfh_on_index(self, normal, radius, max_nn)

    def icp(self, source, max_correspondence_distance, **kwargs):
        """``register.icp`` with this cloud as the target: one index serves many sources.  -> ``IcpResult``."""
        from .register import icp
        return icp(source, self, max_correspondence_distance, **kwargs)


# ---- voxel downsampling ------------------------------------------------------------------------------------------------------------
class VoxelDownsample:
    """Result of ``voxel_downsample``: ``xyz`` [V, 3], ``normal`` / ``sensor`` / ``color`` ([V, C] or None), ``count`` int32 [V] points
    per voxel, ``inverse`` int64 [N] = the output row of every input point, ``index`` int64 [V] = the representative input point
    (``reduce='nearest'`` only, else None).  Rows are in ascending voxel-key order."""

    def __init__(self, xyz, normal, sensor, color, count, inverse, index):
        self.xyz, self.normal, self.sensor, self.color, self.count, self.inverse, self.index = xyz, normal, sensor, color, count, inverse, index

    def __len__(self):
        return int(self.xyz.shape[0])


def voxel_runs(xyz, voxel_size):
    """The cloud grouped by voxel: (order int32 [N] = point indices sorted by voxel key -- stable, so ascending inside a voxel --,
    keys int64 [V] ascending, start / end int32 [V] = every voxel's run in ``order``).  Voxel of a point:
    floor(fl32(x) * inv_w0_f32(voxel_size)) per axis, the hierarchy's definition (nksr_point_keys)."""
    n, dev = xyz.shape[0], xyz.device
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    call('nksr_point_keys', ptr(xyz), n, inv_w0_f32(voxel_size), ptr(keys), stream())
    ks, order = ops.sort_pairs(keys, torch.arange(n, dtype=torch.int32, device=dev))
    _, s, ukeys, _ = ops.sorted_runs(ks, keys=True)          # (Morton keys are below 2^63: every key counts)
    return order, ukeys, s[:-1], s[1:]


def voxel_reduce(order, start, end, xyz, attr=None, nearest=False, group=0):
    """csrc/cloud.hip: -> (mean xyz [V, 3], mean attr [V, C] or None, count int32 [V], nearest int32 [V] or None = the position in
    ``order`` of every run's point nearest its mean).  ``group``: voxels per wavefront, 0 = chosen from V."""
    n, nv, dev = xyz.shape[0], start.numel(), xyz.device
    c = 0 if attr is None else int(attr.shape[1])
    mean = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    amean = torch.empty((nv, c), dtype=torch.float32, device=dev) if c else None
    count = torch.empty(nv, dtype=torch.int32, device=dev)
    near = torch.empty(nv, dtype=torch.int32, device=dev) if nearest else None
    call('nksr_voxel_reduce', ptr(order), n, ptr(start), ptr(end), nv, ptr(xyz), ptr(attr) if c else None, c, int(group), ptr(mean),
         ptr(amean), ptr(count), ptr(near), stream())
    return mean, amean, count, near


def voxel_downsample(xyz, voxel_size, normal=None, sensor=None, color=None, reduce='mean'):
    """One point per occupied voxel of size ``voxel_size``.  ``reduce='mean'``: position and every attribute are the mean over the
    voxel's points; a mean normal is scaled back to unit length (one shorter than 1e-12 -- opposing normals -- is replaced by the normal
    of the voxel's lowest-index point).  ``reduce='nearest'``: the input point nearest the mean (the lowest index on a tie) stands for
    the voxel, with its own attributes.  -> ``VoxelDownsample``."""
    if reduce not in ('mean', 'nearest'):
        raise ValueError("voxel_downsample: reduce must be 'mean' or 'nearest' (got %r)" % (reduce,))
    voxel_size = cloud_input.positive(voxel_size, 'voxel_downsample', 'voxel_size')
    xyz = _check_points(xyz, voxel_size)
    n, dev = xyz.shape[0], xyz.device
    given = [(name, a) for name, a in (('normal', normal), ('sensor', sensor), ('color', color)) if a is not None]
    for name, a in given:
        if a.dim() != 2 or a.shape[0] != n or a.device != dev:
            raise RuntimeError('voxel_downsample: %s must be a [N, C] tensor on the device of xyz' % name)
    if n == 0:
        empty = {name: a.to(torch.float32).reshape(0, a.shape[1]) for name, a in given}
        return VoxelDownsample(xyz, empty.get('normal'), empty.get('sensor'), empty.get('color'), torch.empty(0, dtype=torch.int32, device=dev),
                               torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev) if reduce == 'nearest' else None)
    attr = torch.cat([a.to(torch.float32) for _, a in given], dim=1).contiguous() if given else None
    order, ukeys, start, end = voxel_runs(xyz, voxel_size)
    nearest = reduce == 'nearest'
    mean, amean, count, near = voxel_reduce(order, start, end, xyz, attr, nearest=nearest)
    nv = ukeys.numel()
    inverse = torch.empty(n, dtype=torch.int64, device=dev)
    inverse[order.long()] = torch.repeat_interleave(torch.arange(nv, device=dev), (end - start).long(), output_size=n)
    index = None
    if nearest:
        index = order.long()[near.long()]
        mean = xyz[index]
        amean = attr[index] if attr is not None else None
    out, col = {'normal': None, 'sensor': None, 'color': None}, 0
    for name, a in given:
        out[name] = amean[:, col:col + a.shape[1]].contiguous()
        col += a.shape[1]
    if out['normal'] is not None and not nearest:
        m = out['normal'].double()
        length = m.norm(dim=1, keepdim=True)
        first = normal.to(torch.float32)[order.long()[start.long()]]
        out['normal'] = torch.where(length < 1e-12, first, (m / length.clamp_min(1e-300)).float())
    return VoxelDownsample(mean, out['normal'], out['sensor'], out['color'], count, inverse, index)


# ---- outlier masks -----------------------------------------------------------------------------------------------------------------
def radius_outlier_mask(xyz, radius, min_neighbors):
    """bool [N]: True where a point has at least ``min_neighbors`` OTHER points within ``radius``."""
    m = int(min_neighbors)
    if xyz.shape[0] == 0 or m <= 0:
        require_gpu(xyz.device)
        return torch.ones(xyz.shape[0], dtype=torch.bool, device=xyz.device)
    return CloudIndex(xyz).radius_count(radius, cap=m, exclude_self=True) >= m


def statistical_outlier_mask(xyz, k=16, std_ratio=2.0):
    """bool [N]: True where m_i <= mu + std_ratio * sigma, m_i = the mean distance of point i to its k nearest other points, mu / sigma =
    mean and sample standard deviation (N - 1) of m, reduced in fp64 on the device."""
    m = CloudIndex(xyz).mean_knn_distance(k).double()
    sigma = m.std(unbiased=True) if m.numel() > 1 else m.new_zeros(())
    return m <= m.mean() + float(std_ratio) * sigma
