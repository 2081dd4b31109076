"""Mesh quality metrics on the GPU: ``MeshEvaluator`` (the scorer the reference's test loop calls, models/nksr_net.py:298-310).

A mesh is scored against an oriented ground-truth cloud through area-uniform samples of its surface:
  completeness  mean distance of every ground-truth point to its nearest sample       accuracy   the same from the samples to the truth
  chamfer-L1    mean of the two (chamfer-L2: of their squares)                         normals    mean |n . n_nn| over both directions
  f-score       2 p r / (p + r), p = share of samples within t of the truth, r = share of the truth within t of a sample,
                t = 0.01 ('f-score'), 0.015, 0.02 and 0.1 ('-outdoor')
Every stage runs on the GPU (csrc/metrics.hip: face areas, the fp64 area CDF, the counter-based sampler, the fixed-order reduce;
its k_nn_metrics on the octree search of csrc/knn_topk_dev.h: the exact nearest neighbour of every query over an octree of the other cloud).  Coordinates are recentred in float64
by the centre of the target's bounding box before they are rounded to float32, so scenes far from the origin keep their precision
(nksr_amd/mesh_input.py, which turns every caller's array into a checked device tensor).
Results are bitwise reproducible: the samples depend on (seed, index) only and no sum uses float atomics.
``o3d-iou`` (requested through ``metric_names``) is the volumetric IoU against ``onet_samples`` = (points, occupancy): the mesh's
occupancy of the points by ray parity (``MeshQuery``, nksr_amd/mesh_query.py: a BVH over the triangles, csrc/meshquery.hip), then
sum(pd & gt) / (sum(pd | gt) + 1e-6) with integer counts, as in the reference (metrics.py:182-190).
"""
import numpy as np
import torch

from ._lib import METRIC_FIELDS, NN_BLOCK, call, ptr, stream, with_tmp
from .density import bbox_center
from .mesh_input import bbox_centre, faces, gpu_device, is64, normals32, recentre
from .mesh_query import MeshQuery, mesh_occupancy  # noqa: F401  (re-exported: nksr.metrics.MeshQuery)
from .mesh_geometry import MeshGeometry  # noqa: F401  (re-exported: nksr.metrics.MeshGeometry)
from .mesh_simplify import MeshSimplifier  # noqa: F401  (re-exported: nksr.metrics.MeshSimplifier)
from .mesh_boundary import MeshBoundary  # noqa: F401  (re-exported: nksr.metrics.MeshBoundary)
from .mesh_clip import MeshClipper  # noqa: F401  (re-exported: nksr.metrics.MeshClipper)
from .mesh_raster import MeshRasterizer  # noqa: F401  (re-exported: nksr.metrics.MeshRasterizer)
from .mesh_slice import MeshSlicer  # noqa: F401  (re-exported: nksr.metrics.MeshSlicer)
from .mesh_topology import MeshTopology  # noqa: F401  (re-exported: nksr.metrics.MeshTopology)
from .neighbours import PointGrid, PointPyramid, choose_cell_size

THRESHOLDS = (0.01, 0.015, 0.02, 0.002, 0.1)    # NKSR_METRIC_THRESHOLDS; 'f-score' at [0], '-15' [1], '-20' [2], '-outdoor' [4]
MAX_RING = 4                                    # rings per pyramid level before a query climbs (nksr_nn_metrics)
_KEY_CELLS = float(1 << 18)                     # |coordinate| / cell stays below this: cell indices far inside the 21-bit key range
IOU_RAYS = 3                                    # rays per ONet sample of 'o3d-iou' (majority of three parities)


# ---- stages (nksr_amd/tools/prof_metrics.py times them one by one) -------------------------------------------------------------------
def face_cdf(v32, f):
    """(unit face normals [F, 3] float32, inclusive float64 CDF of the face areas [F])."""
    nf, dev = f.shape[0], v32.device
    normal = torch.empty((nf, 3), dtype=torch.float32, device=dev)
    area = torch.empty(nf, dtype=torch.float64, device=dev)
    cdf = torch.empty(nf, dtype=torch.float64, device=dev)
    call('nksr_mesh_face_areas', ptr(v32), v32.shape[0], ptr(f), is64(f), nf, ptr(normal), ptr(area), stream())
    if nf:
        with_tmp('nksr_inclusive_sum_f64', dev, ptr(area), ptr(cdf), nf, stream())
    return normal, cdf


def sample_from_cdf(v32, f, fnormal, cdf, n, seed):
    """n samples of the mesh (points [n, 3], their faces' unit normals [n, 3], face index [n] int64)."""
    dev = v32.device
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int64, device=dev)
    call('nksr_mesh_sample', ptr(v32), v32.shape[0], ptr(f), is64(f), f.shape[0], ptr(cdf), ptr(fnormal), n,
         int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(xyz), ptr(nrm), ptr(face), stream())
    return xyz, nrm, face


class Cloud:
    """A float32 cloud ready for nearest-neighbour queries: Morton-sorted points (+ normals) under a ``PointPyramid``."""

    def __init__(self, xyz, normal=None):
        if xyz.shape[0] == 0:
            raise ValueError('nearest-neighbour target is empty')
        cell = choose_cell_size(xyz, 4)
        lo, hi, _ = bbox_center(xyz)
        reach = float(torch.maximum(lo.abs(), hi.abs()).max())
        cell = max(cell, reach / _KEY_CELLS, 1e-30)
        self.pyramid = PointPyramid(PointGrid(xyz, cell))
        pg = self.pyramid.pg
        self.xyz = pg.xyz
        self.normal = normal[pg.perm].contiguous() if normal is not None else None
        self.n = xyz.shape[0]

    def nearest(self, query, qnormal=None, dist=None, dot=None, sums=True):
        """One nksr_nn_metrics pass of `query` against this cloud: fills `dist` / `dot` ([nq] float32, optional) and returns the
        float64 [8] sums (d, d^2, dot, counts of d <= THRESHOLDS) when `sums`.  The dots need both normal sets."""
        nq = query.shape[0]
        dev = query.device
        both = qnormal is not None and self.normal is not None
        out = torch.zeros(METRIC_FIELDS, dtype=torch.float64, device=dev)
        if nq == 0:
            return out if sums else None
        rows = (nq + NN_BLOCK - 1) // NN_BLOCK
        parts = torch.empty((rows, METRIC_FIELDS), dtype=torch.float64, device=dev) if sums else None
        p = self.pyramid
        call('nksr_nn_metrics', p.struct, ptr(p.top_keys), p.top_keys.numel(), ptr(self.normal if both else None), ptr(query),
             ptr(qnormal if both else None), nq, MAX_RING, ptr(dist), ptr(dot if both else None), ptr(parts), stream())
        if not sums:
            return None
        call('nksr_metric_reduce', ptr(parts), rows, ptr(out), stream())
        return out


def metrics_from_sums(comp, acc, n_tgt, n_pred, with_normals):
    """The reference's metric dict from the two float64 [8] sum vectors (gt -> samples, samples -> gt)."""
    c = comp.cpu().numpy() / n_tgt
    a = acc.cpu().numpy() / n_pred
    recall, precision = c[3:], a[3:]
    f = [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)]
    nan = float('nan')
    out = {'completeness': c[0], 'accuracy': a[0], 'normals completeness': c[2] if with_normals else nan,
           'normals accuracy': a[2] if with_normals else nan, 'normals': 0.5 * (c[2] + a[2]) if with_normals else nan,
           'completeness2': c[1], 'accuracy2': a[1], 'chamfer-L2': 0.5 * (c[1] + a[1]), 'chamfer-L1': 0.5 * (c[0] + a[0]),
           'f-precision': precision[0], 'f-recall': recall[0], 'f-score': f[0], 'f-score-15': f[1], 'f-score-20': f[2],
           'f-precision-outdoor': precision[4], 'f-recall-outdoor': recall[4], 'f-score-outdoor': f[4]}
    return {k: float(v) for k, v in out.items()}


# ---- public API ----------------------------------------------------------------------------------------------------------------------
def sample_surface(v, f, n, seed=0, device=None):
    """n area-uniform samples of the mesh (v [V, 3], f [F, 3] int32 / int64) on the GPU, in float32 coordinates as given:
    (points [n, 3], unit normals of their triangles [n, 3], face index [n] int64).  Sample i depends on (seed, i) only
    (Philox4x32-10, include/nksr_hip.h ``nksr_mesh_sample``); triangles of zero area are never picked."""
    dev = gpu_device(device, like=v)
    n = int(n)
    if n < 0:
        raise ValueError('sample_surface: n must be >= 0')
    v32 = recentre(v, np.zeros(3), dev, 'vertices')
    ff = faces(f, v32.shape[0], dev, cast_float=True, check_range=True)
    fn, cdf = face_cdf(v32, ff)
    if n and (ff.shape[0] == 0 or not float(cdf[-1]) > 0.0):
        raise ValueError('sample_surface: the mesh has no area')
    return sample_from_cdf(v32, ff, fn, cdf, n, seed)


def distance_p2p(src, nsrc, tgt, ntgt, device=None):
    """Nearest-neighbour distance of every src point to tgt and |unit n_src . unit n_nn| (a zero normal gives 0) as [N] float32
    tensors on the GPU; dot is None unless both normal sets are given.  Exact: every query gets its nearest target point."""
    dev = gpu_device(device)
    centre = bbox_centre(tgt)
    t = recentre(tgt, centre, dev, 'tgt')
    q = recentre(src, centre, dev, 'src')
    cloud = Cloud(t, normals32(ntgt, t.shape[0], dev, 'ntgt'))
    qn = normals32(nsrc, q.shape[0], dev, 'nsrc')
    dist = torch.empty(q.shape[0], dtype=torch.float32, device=dev)
    dot = torch.empty(q.shape[0], dtype=torch.float32, device=dev) if (qn is not None and cloud.normal is not None) else None
    cloud.nearest(q, qn, dist=dist, dot=dot, sums=False)
    return dist, dot


class MeshEvaluator:
    """GPU counterpart of the reference's ``metrics.MeshEvaluator`` (same metric names, thresholds and sample counts)."""

    ESSENTIAL_METRICS = ['chamfer-L1', 'f-score', 'normals']
    ALL_METRICS = ['completeness', 'accuracy', 'normals completeness', 'normals accuracy', 'normals', 'completeness2', 'accuracy2',
                   'chamfer-L2', 'chamfer-L1', 'f-precision', 'f-recall', 'f-score', 'f-score-15', 'f-score-20']

    def __init__(self, n_points=100000, metric_names=ALL_METRICS, device=None):
        self.n_points = int(n_points)
        self.metric_names = list(metric_names)
        self.device = gpu_device(device)

    def _filter(self, d):
        return {k: d[k] for k in self.metric_names if k in d}

    def _nan(self):
        return {k: float('nan') for k in self.metric_names}

    def eval_mesh(self, mesh, pointcloud_tgt, normals_tgt, onet_samples=None, seed=0):
        """Metrics of `mesh` (a MeshingResult or anything with .v / .f) against the target cloud: ``n_points`` samples of the
        surface, scored with ``evaluate``; with 'o3d-iou' in ``metric_names``, also the IoU of the mesh's occupancy of
        ``onet_samples`` = (points [N, 3], occupancy [N], nonzero = inside) against theirs.  A mesh without area scores NaN
        throughout."""
        want_iou = 'o3d-iou' in self.metric_names
        if onet_samples is not None and not want_iou:
            raise NotImplementedError("onet_samples given but 'o3d-iou' is not in metric_names: add 'o3d-iou' to metric_names to "
                                      "score them")
        if want_iou and onet_samples is None:
            raise ValueError("'o3d-iou' needs onet_samples = (points, occupancy)")
        dev = self.device
        centre = bbox_centre(pointcloud_tgt)
        v32 = recentre(mesh.v, centre, dev, 'mesh.v')
        ff = faces(mesh.f, v32.shape[0], dev, cast_float=True, check_range=True)
        if ff.shape[0] == 0 or self.n_points == 0:
            return self._nan()
        fn, cdf = face_cdf(v32, ff)
        if not float(cdf[-1]) > 0.0:
            return self._nan()
        p, n, _ = sample_from_cdf(v32, ff, fn, cdf, self.n_points, seed)
        t = recentre(pointcloud_tgt, centre, dev, 'pointcloud_tgt')
        out = self._evaluate(p, n, t, normals32(normals_tgt, t.shape[0], dev, 'normals_tgt'))
        if want_iou:
            out['o3d-iou'] = self._iou(MeshQuery.recentred(v32, ff, centre), onet_samples)
        return out

    def _iou(self, query, onet_samples):
        """sum(pd & gt) / (sum(pd | gt) + 1e-6), integer counts (the reference's formula, metrics.py:186-188)."""
        if len(onet_samples) != 2:
            raise ValueError('onet_samples: expected (points, occupancy)')
        pts, occ = onet_samples
        gt = occ.detach() if isinstance(occ, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(occ)))
        gt = (gt.to(self.device) != 0).reshape(-1)
        pd = query.occupancy(pts, rays=IOU_RAYS)
        if gt.shape[0] != pd.shape[0]:
            raise ValueError('onet_samples: %d occupancy values for %d points' % (gt.shape[0], pd.shape[0]))
        inter, union = int((pd & gt).sum()), int((pd | gt).sum())
        return inter / (union + 1.0e-6)

    def evaluate(self, pointcloud, pointcloud_tgt, normals=None, normals_tgt=None):
        """The metric dict of a given sample set against the target (the reference's ``_evaluate``)."""
        dev = self.device
        centre = bbox_centre(pointcloud_tgt)
        p = recentre(pointcloud, centre, dev, 'pointcloud')
        t = recentre(pointcloud_tgt, centre, dev, 'pointcloud_tgt')
        return self._evaluate(p, normals32(normals, p.shape[0], dev, 'normals'), t, normals32(normals_tgt, t.shape[0], dev, 'normals_tgt'))

    def _evaluate(self, p, pn, t, tn):
        if p.shape[0] == 0:
            return self._nan()
        if t.shape[0] == 0:
            raise ValueError('pointcloud_tgt is empty')
        pred, gt = Cloud(p, pn), Cloud(t, tn)
        comp = pred.nearest(gt.xyz, gt.normal)          # queries in the Morton order of their own pyramid
        acc = gt.nearest(pred.xyz, pred.normal)
        return self._filter(metrics_from_sums(comp, acc, gt.n, pred.n, pn is not None and tn is not None))
