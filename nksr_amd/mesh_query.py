"""Triangle-mesh queries on the GPU: ``MeshQuery`` (occupancy, closest point, signed distance), the counterpart of the
reference's ``vis.RayDistanceQuery`` (metrics.py:182-190), and the ``o3d-iou`` of ``metrics.MeshEvaluator``.

    q = MeshQuery(v, f)                       # builds the BVH once; v / f numpy or torch, f int32 / int64
    occ = q.occupancy(points, rays=3)         # [N] bool on the GPU
    d, face = q.distance(points)              # [N] float32, [N] int64 (closest_point=True adds [N, 3])
    sd = q.signed_distance(points, rays=3)    # -d inside, +d outside

The tree is a linear BVH over the triangles (csrc/meshquery.hip).  Occupancy casts ``rays`` half-lines
(1, 3, 5 or 7 fixed, non-axis-aligned directions) from every query and counts every crossing with a watertight test whose signs are
exact and whose ties on shared edges and vertices are broken per edge: on a closed mesh each ray's parity is exact, and a query is
inside when most of its rays cross an odd number of times.  Coordinates are recentred in float64 by the centre of the mesh's bounding
box before they are rounded to float32 (nksr_amd/mesh_input.py; faces of any dtype are indices, one outside [0, V) is an error).
A mesh without faces has nothing inside and every distance is inf.
"""
import numpy as np
import torch

from . import mesh_input, ops
from ._lib import BVH_LEAF_FLOATS, BVH_MAX_FACES, BVH_MAX_RAYS, BVH_NODE_FLOATS, BVH_STACK, BvhT, call, ptr, stream
from .density import bbox_center
from .mesh_input import bbox_centre, gpu_device, is64, recentre, rows3


def _check_rays(rays):
    if isinstance(rays, bool) or not isinstance(rays, (int, np.integer)) or rays < 1 or rays > BVH_MAX_RAYS or rays % 2 == 0:
        raise ValueError('rays must be an odd count in [1, %d], got %r' % (BVH_MAX_RAYS, rays))
    return int(rays)


# ---- build stages (nksr_amd/tools/prof_mesh_query.py times them one by one) ------------------------------------------------------------
def morton(xyz, box, faces=None, nv=None):
    """(Morton codes [n] int64, indices [n] int32) of the face centroids (faces given) or of the points, in box (device [6])."""
    n = faces.shape[0] if faces is not None else xyz.shape[0]
    codes = torch.empty(n, dtype=torch.int64, device=xyz.device)
    index = torch.empty(n, dtype=torch.int32, device=xyz.device)
    call('nksr_bvh_morton', ptr(xyz), xyz.shape[0] if nv is None else nv, ptr(faces), is64(faces) if faces is not None else 0, n, ptr(box),
         ptr(codes), ptr(index), stream())
    return codes, index


def sort_codes(codes, index):
    """(sorted codes, index in their order): one radix sort of the 63-bit keys."""
    return ops.sort_pairs(codes, index, end_bit=63)


class Bvh:
    """Device arrays of one tree (``nksr_bvh_t``)."""

    def __init__(self, nf, box, dev):
        self.nf = nf
        self.box = box
        self.nodes = torch.empty((max(nf - 1, 1), BVH_NODE_FLOATS), dtype=torch.float32, device=dev)
        self.leaves = torch.empty((max(nf, 1), BVH_LEAF_FLOATS), dtype=torch.float32, device=dev)
        self.depth_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.depth = 0
        self.struct = BvhT(nf, 0, 0, ptr(self.nodes), ptr(self.leaves), ptr(box), ptr(self.depth_dev))


def build_nodes(bvh, codes_sorted):
    """Internal nodes of the tree; returns the parent words [2F - 1] the refit climbs."""
    parent = torch.empty(max(2 * bvh.nf - 1, 1), dtype=torch.int32, device=codes_sorted.device)
    call('nksr_bvh_nodes', ptr(codes_sorted), ptr(parent), bvh.struct, stream())
    return parent


def refit(bvh, v32, faces, order, parent):
    """Leaf records and every box, bottom up; bvh.depth_dev receives the depth (read by ``finish``)."""
    work = torch.empty(max(2 * (bvh.nf - 1), 1), dtype=torch.int32, device=v32.device)
    call('nksr_bvh_refit', ptr(v32), v32.shape[0], ptr(faces), is64(faces), ptr(order), ptr(parent), ptr(work),
         bvh.struct, stream())


def finish(bvh):
    """Reads the depth back (syncs) and refuses a tree deeper than the traversal stack."""
    bvh.depth = int(bvh.depth_dev.item()) if bvh.nf else 0
    bvh.struct.depth = bvh.depth
    if bvh.depth > BVH_STACK:
        raise RuntimeError('mesh query: the BVH is %d levels deep, the traversal stack holds %d' % (bvh.depth, BVH_STACK))
    return bvh


def build_bvh(v32, faces):
    """The whole build: box, codes, sort, nodes, refit (v32 [V, 3] float32 and faces [F, 3] on the GPU, indices checked)."""
    nf, dev = faces.shape[0], v32.device
    if nf > BVH_MAX_FACES:
        raise ValueError('mesh query: %d faces, at most 2^30' % nf)
    if nf == 0:
        return Bvh(0, torch.zeros(6, dtype=torch.float32, device=dev), dev)
    lo, hi, _ = bbox_center(v32)
    box = torch.cat([lo, hi]).contiguous()
    bvh = Bvh(nf, box, dev)
    codes, index = morton(v32, box, faces, v32.shape[0])
    ks, order = sort_codes(codes, index)
    parent = build_nodes(bvh, ks)
    refit(bvh, v32, faces, order, parent)
    return finish(bvh)


class MeshQuery:
    """Occupancy and distance queries against one triangle mesh (v [V, 3], f [F, 3] int32 / int64), on the GPU."""

    def __init__(self, v, f, device=None):
        dev = gpu_device(device, like=v)
        vv = v if isinstance(v, torch.Tensor) else np.asarray(v)
        rows3(vv, 'vertices')
        centre = bbox_centre(vv) if vv.shape[0] else np.zeros(3)
        v32 = recentre(vv, centre, dev, 'vertices')
        self._init(build_bvh(v32, mesh_input.faces(f, v32.shape[0], dev, cast_float=True, check_range=True)), centre)

    @classmethod
    def recentred(cls, v32, faces, centre):
        """A query over vertices already recentred by ``centre`` (float32 on the GPU, faces checked): MeshEvaluator's path."""
        return cls.from_bvh(build_bvh(v32, faces), centre)

    @classmethod
    def from_bvh(cls, bvh, centre):
        """A query over a finished tree whose vertices were recentred by ``centre``."""
        q = cls.__new__(cls)
        q._init(bvh, np.asarray(centre, np.float64))
        return q

    def _init(self, bvh, centre):
        self.device = bvh.nodes.device
        self.centre = centre
        self.n_faces = int(bvh.nf)
        self.bvh = bvh
        self.depth = bvh.depth

    # ---- queries ------------------------------------------------------------------------------------------------------------------
    def _queries(self, points):
        """Recentred float32 [N, 3] on the GPU."""
        return recentre(points, self.centre, self.device, 'points')

    def _order(self, q):
        """Morton order of the queries ([N] int32, None when there is nothing to walk).  Occupancy walks them in this order: 1e6
        ONet-style queries of the 2.3 M-face scene take 3.3 ms at rays = 3 sorted against 5.6 ms unsorted, the sort 0.3 ms.  The
        closest-point search walks them as given: sorted, it was slower (11.8 against 6.9 ms for 1e5 queries of the configs[1]
        sphere, 99.9 against 96.7 ms on the scene)."""
        if q.shape[0] == 0 or self.n_faces == 0:
            return None
        codes, index = morton(q, self.bvh.box)
        return sort_codes(codes, index)[1]

    def _occupancy(self, q, order, rays, counts=False):
        n = q.shape[0]
        inside = torch.zeros(n, dtype=torch.bool, device=self.device)
        cnt = torch.zeros((n, rays), dtype=torch.int32, device=self.device) if counts else None
        if n and self.n_faces:
            call('nksr_mesh_occupancy', self.bvh.struct, ptr(q), n, ptr(order), rays, ptr(inside), ptr(cnt), stream())
        return inside, cnt

    def _closest(self, q, order, closest_point=False):
        n = q.shape[0]
        dist = torch.full((n,), float('inf'), dtype=torch.float32, device=self.device)
        face = torch.full((n,), -1, dtype=torch.int64, device=self.device)
        pt = torch.full((n, 3), float('nan'), dtype=torch.float32, device=self.device) if closest_point else None
        if n and self.n_faces:
            call('nksr_mesh_closest', self.bvh.struct, ptr(q), n, ptr(order), ptr(dist), ptr(face), ptr(pt), stream())
        return dist, face, pt

    def occupancy(self, points, rays=3):
        """[N] bool: inside the mesh, by the parity of ``rays`` half-lines from each point (1, 3, 5 or 7; majority vote)."""
        rays = _check_rays(rays)
        q = self._queries(points)
        return self._occupancy(q, self._order(q), rays)[0]

    def crossings(self, points, rays=3):
        """[N, rays] int32: the number of triangles each ray crosses (every crossing along the half-line)."""
        rays = _check_rays(rays)
        q = self._queries(points)
        return self._occupancy(q, self._order(q), rays, counts=True)[1]

    def distance(self, points, closest_point=False):
        """(distance [N] float32, closest face [N] int64, and with ``closest_point`` the closest point [N, 3] float32 in the caller's
        coordinates).  Exact search; a tie goes to the smaller face index.  No faces: inf and -1."""
        dist, face, pt = self._closest(self._queries(points), None, closest_point)
        if not closest_point:
            return dist, face
        pt = (pt.double() + torch.from_numpy(self.centre).to(self.device)).float()
        return dist, face, pt

    def signed_distance(self, points, rays=3):
        """[N] float32: the distance, negative inside (occupancy with ``rays``)."""
        rays = _check_rays(rays)
        q = self._queries(points)
        inside = self._occupancy(q, self._order(q), rays)[0]
        dist = self._closest(q, None)[0]
        return torch.where(inside, -dist, dist)


def mesh_occupancy(v, f, points, rays=3, device=None):
    """One-shot ``MeshQuery(v, f, device).occupancy(points, rays)``."""
    _check_rays(rays)
    return MeshQuery(v, f, device).occupancy(points, rays)
