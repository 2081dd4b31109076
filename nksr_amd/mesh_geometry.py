"""Triangle-mesh geometry on the GPU: ``MeshGeometry`` (vertex adjacency, vertex normals, vertex areas, Gaussian and mean curvature,
Laplacian / Taubin smoothing).

    g = MeshGeometry(v, f)                  # v numpy / torch fp32 / fp64 on any device, f int32 / int64 (float / bool faces refused)
    g = MeshGeometry.from_topology(t)       # reuse a MeshTopology's tables; g.topology is t
    g.neighbour_start [V + 1], g.neighbours [2E] int32      # vertex adjacency, each row ascending; g.vertex_degree [V]
    g.vertex_kind [V] uint8                 # 0 interior, 1 on a boundary edge, 2 unreferenced
    g.vertex_normals(weighting='angle')     # or 'area'; [V, 3] unit, dtype of v; (0, 0, 0) where the sum vanishes / unreferenced
    g.vertex_areas()                        # [V] fp64, barycentric: a third of each incident valid face
    g.gaussian_curvature(integrated=False)  # [V] fp64: angle defect 2 pi - sum theta (integrated) or that over the vertex area
    g.mean_curvature()                      # [V] fp64, signed, positive on an outward-oriented sphere
    g.smooth(iterations, method='taubin', lam=0.5, mu=-0.53, boundary='fixed', fixed=None)      # -> new v (GPU tensor)

Definitions (kernels in csrc/meshgeom.hip):
  Laplacian step   x_i <- x_i + w (mean_{j in N(i)} x_j - x_i), uniform weights over the DISTINCT neighbours.  method='laplacian':
                   ``iterations`` steps with w = lam; method='taubin': ``iterations`` pairs, a lam step then a mu step (Taubin's
                   lambda | mu filter; the defaults are Open3D's).  0 < lam <= 1, and for taubin mu < -lam, else ValueError;
                   iterations = 0 returns a copy.
  boundary         'fixed': vertices of kind 1 do not move.  'curve': a kind-1 vertex averages only the neighbours it reaches over
                   boundary-class edges, so an open border is smoothed as a curve and does not pull inward (chunk-open and terrain
                   meshes).  'free': no special case.
  fixed            optional [V] bool mask of further pinned vertices.  Unreferenced vertices never move; vertices on non-manifold
                   edges are ordinary.
  normals          angle-weighted: sum theta_corner n_face; area-weighted: sum area n_face (n_face the unit face normal), normalised.
  vertex area      A_i = a third of the area of every incident valid face.
  Gaussian         angle defect 2 pi - sum of the incident corner angles (integrated), or that over A_i.
  mean curvature   Delta x_i = (1 / 2 A_i) sum_j (cot alpha_ij + cot beta_ij) (x_j - x_i); the weight of an edge is the sum, over ALL
                   valid faces on it, of the cotangent of the opposite corner, so non-manifold edges are covered.
                   H_i = |Delta x_i| / 2 * sgn(-Delta x_i . n_i) with the angle-weighted normal.
  NaN              both curvatures at vertices of kind 1 or 2 and where A_i = 0 (an angle defect at a border means something else).
  invalid faces    (as MeshTopology defines them) contribute nothing anywhere.
Precision: positions are read in the caller's precision; all state (the smoothing ping-pong buffers, corner angles, cotangents,
accumulators) is fp64, with one rounding to the caller's dtype at the very end -- fp64 vertices with an offset of 1e6 smooth without
recentring.  Every result repeats bit for bit: there is no floating-point atomic, every sum runs in the fixed order of its sorted row
(neighbours ascending, corners ascending, half-edges of an edge in ascending id).  Limits: as MeshTopology (V < 2^31, F <= 2^30);
offsets into the 2E and 3F arrays are uint32 stored in int32 tensors, like ``edge_start``.
"""
import math

import torch

from . import ops
from ._lib import (GEOM_CURVE, GEOM_FIXED, GEOM_FREE, GEOM_INTERIOR, GEOM_WEIGHT_ANGLE, GEOM_WEIGHT_AREA, call, ptr, stream)
from .mesh_input import is64
from .mesh_topology import MeshTopology

WEIGHTINGS = {'angle': GEOM_WEIGHT_ANGLE, 'area': GEOM_WEIGHT_AREA}
BOUNDARIES = {'fixed': GEOM_FIXED, 'curve': GEOM_CURVE, 'free': GEOM_FREE}
METHODS = ('taubin', 'laplacian')


# ---- stages (nksr_amd/tools/prof_mesh_geometry.py times them one by one) ------------------------------------------------------------
def adjacency(edges, edge_classes, vertex_ref, nv):
    """(neighbour_start [V + 1], neighbours [2E], neighbour_edge [2E] int32, neighbour_class [2E], vertex_kind [V] uint8)."""
    ne, dev = edges.shape[0], edges.device
    keys = torch.empty(2 * ne, dtype=torch.int64, device=dev)
    ids = torch.empty(2 * ne, dtype=torch.int32, device=dev)
    call('nksr_geom_directed_keys', ptr(edges), ne, nv, ptr(keys), ptr(ids), stream())
    ks, ids_sorted = ops.sort_pairs(keys, ids, end_bit=32 + int(nv).bit_length())
    start = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    nbr = torch.empty(2 * ne, dtype=torch.int32, device=dev)
    nbr_edge = torch.empty(2 * ne, dtype=torch.int32, device=dev)
    nbr_class = torch.empty(2 * ne, dtype=torch.uint8, device=dev)
    kind = torch.empty(nv, dtype=torch.uint8, device=dev)
    call('nksr_geom_adjacency', ptr(ks), ptr(ids_sorted), ne, nv, ptr(vertex_ref), ptr(edge_classes), ptr(start), ptr(nbr), ptr(nbr_edge),
         ptr(nbr_class), ptr(kind), stream())
    return start, nbr, nbr_edge, nbr_class, kind


def corner_incidence(f, face_valid, nv):
    """(corner_start [V + 1], corner_ids [3F] int32): the corners 3 f + k of valid faces by vertex, ascending inside a row."""
    nf, dev = f.shape[0], f.device
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    ids = torch.empty(3 * nf, dtype=torch.int32, device=dev)
    call('nksr_geom_corner_keys', ptr(f), is64(f), nf, nv, ptr(face_valid), ptr(keys), ptr(ids), stream())
    ks, ids_sorted = ops.sort_pairs(keys, ids, end_bit=max(int(nv).bit_length(), 1))
    start = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    call('nksr_geom_corner_rows', ptr(ks), 3 * nf, nv, ptr(start), stream())
    return start, ids_sorted


def face_pass(x, f, face_valid):
    """(angle [F, 3], cot [F, 3], normal [F, 3], area [F]) fp64 of every face, zeros for an invalid one."""
    nf, nv, dev = f.shape[0], x.shape[0], f.device
    angle, cot, normal = (torch.empty((nf, 3), dtype=torch.float64, device=dev) for _ in range(3))
    area = torch.empty(nf, dtype=torch.float64, device=dev)
    call('nksr_geom_faces', ptr(x), int(x.dtype == torch.float64), nv, ptr(f), is64(f), nf, ptr(face_valid), ptr(angle), ptr(cot), ptr(normal),
         ptr(area), stream())
    return angle, cot, normal, area


class MeshGeometry:
    """Geometry of one triangle mesh (v [V, 3], f [F, 3] int32 / int64) on the GPU; see the module's docstring."""

    def __init__(self, v, f, device=None):
        self._init(MeshTopology(v, f, device))

    @classmethod
    def from_topology(cls, topology):
        """The geometry over the tables of a ``MeshTopology`` that exists already."""
        if not isinstance(topology, MeshTopology):
            raise TypeError('from_topology: expected a MeshTopology, got %s' % type(topology).__name__)
        g = cls.__new__(cls)
        g._init(topology)
        return g

    def _init(self, t):
        self.topology, self.device = t, t.device
        self.v, self.f = t.v, t.f
        self.x = t.v if t.v.dtype in (torch.float32, torch.float64) else t.v32        # what the kernels read
        self.n_vertices, self.n_faces = t.n_vertices, t.n_faces
        (self.neighbour_start, self.neighbours, self.neighbour_edge, self.neighbour_class,
         self.vertex_kind) = adjacency(t.edges, t.edge_classes, t.vertex_ref, t.n_vertices)
        self._corners = self._faces = self._edge_weight = None
        self._sums = {}

    @property
    def vertex_degree(self):
        """[V] int64: the number of distinct neighbours."""
        s = self.neighbour_start.long() & 0xFFFFFFFF
        return s[1:] - s[:-1]

    # ---- cached stages ----
    def corners(self):
        if self._corners is None:
            self._corners = corner_incidence(self.f, self.topology.face_valid, self.n_vertices)
        return self._corners

    def faces(self):
        if self._faces is None:
            self._faces = face_pass(self.x, self.f, self.topology.face_valid)
        return self._faces

    def edge_weights(self):
        """[E] fp64 cotangent weight of every unique edge."""
        if self._edge_weight is None:
            t, ne = self.topology, self.topology.edges.shape[0]
            self._edge_weight = torch.empty(ne, dtype=torch.float64, device=self.device)
            call('nksr_geom_edge_weights', ptr(t._ids_sorted), ptr(t._table.edge_start), ne, self.n_faces, ptr(self.faces()[1]),
                 ptr(self._edge_weight), stream())
        return self._edge_weight

    def vertex_sums(self, weighting='angle'):
        """(unit normal [V, 3], area [V], angle sum [V]) fp64 from one gather over the corner rows."""
        if weighting not in WEIGHTINGS:
            raise ValueError("weighting must be 'angle' or 'area', got %r" % (weighting,))
        if weighting not in self._sums:
            nv, dev = self.n_vertices, self.device
            start, ids = self.corners()
            angle, _, normal, area = self.faces()
            n = torch.empty((nv, 3), dtype=torch.float64, device=dev)
            a = torch.empty(nv, dtype=torch.float64, device=dev)
            s = torch.empty(nv, dtype=torch.float64, device=dev)
            call('nksr_geom_vertex_gather', ptr(start), ptr(ids), nv, self.n_faces, ptr(angle), ptr(normal), ptr(area), WEIGHTINGS[weighting],
                 ptr(n), ptr(a), ptr(s), stream())
            self._sums[weighting] = (n, a, s)
        return self._sums[weighting]

    # ---- results ----
    def vertex_normals(self, weighting='angle'):
        """[V, 3] unit normals in the dtype of v; zero rows where the weighted sum vanishes or the vertex is unreferenced."""
        return self.vertex_sums(weighting)[0].to(self.v.dtype)

    def vertex_areas(self):
        """[V] fp64 barycentric areas."""
        return self.vertex_sums(next(iter(self._sums), 'angle'))[1]

    def _undefined(self):
        return (self.vertex_kind != GEOM_INTERIOR) | ~(self.vertex_areas() > 0)

    def gaussian_curvature(self, integrated=False):
        """[V] fp64: the angle defect (``integrated``) or the defect over the vertex area; NaN at kinds 1, 2 and where the area is 0."""
        _, area, angles = self.vertex_sums(next(iter(self._sums), 'angle'))
        k = 2.0 * math.pi - angles
        if not integrated:
            k = k / area
        return torch.where(self._undefined(), torch.full_like(k, float('nan')), k)

    def _curvature(self, want_laplacian):
        nv, dev = self.n_vertices, self.device
        normal, area, _ = self.vertex_sums('angle')
        lap = torch.empty((nv, 3), dtype=torch.float64, device=dev) if want_laplacian else None
        h = torch.empty(nv, dtype=torch.float64, device=dev)
        call('nksr_geom_curvature', ptr(self.x), int(self.x.dtype == torch.float64), nv, ptr(self.neighbour_start), ptr(self.neighbours),
             ptr(self.neighbour_edge), self.topology.edges.shape[0], ptr(self.edge_weights()), ptr(area), ptr(normal), ptr(self.vertex_kind),
             ptr(lap), ptr(h), stream())
        return lap, h

    def mean_curvature(self):
        """[V] fp64 signed mean curvature (positive on an outward-oriented sphere); NaN as ``gaussian_curvature``."""
        return self._curvature(False)[1]

    def cotangent_laplacian(self):
        """[V, 3] fp64 Delta x (the mean-curvature normal, -2 H n on a smooth surface); NaN rows as ``gaussian_curvature``."""
        return self._curvature(True)[0]

    def smooth(self, iterations, method='taubin', lam=0.5, mu=-0.53, boundary='fixed', fixed=None):
        """New vertex positions [V, 3] (a GPU tensor in the dtype of v) after ``iterations`` Taubin pairs or Laplacian steps; all steps
        are queued on the current stream over two fp64 buffers, without a host synchronisation between them."""
        if method not in METHODS:
            raise ValueError("method must be 'taubin' or 'laplacian', got %r" % (method,))
        if boundary not in BOUNDARIES:
            raise ValueError("boundary must be 'fixed', 'curve' or 'free', got %r" % (boundary,))
        if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
            raise ValueError('iterations must be a non-negative integer, got %r' % (iterations,))
        lam, mu = float(lam), float(mu)
        if not 0.0 < lam <= 1.0:
            raise ValueError('lam must lie in (0, 1], got %r' % (lam,))
        if method == 'taubin' and not mu < -lam:
            raise ValueError('taubin: mu must be below -lam = %r, got %r' % (-lam, mu))
        nv, dev = self.n_vertices, self.device
        mask = None
        if fixed is not None:
            mask = torch.as_tensor(fixed)
            if mask.shape != (nv,):
                raise ValueError('fixed: expected %d flags, got shape %s' % (nv, tuple(mask.shape)))
            mask = (mask.to(dev) != 0).to(torch.uint8).contiguous()
        steps = int(iterations) * (2 if method == 'taubin' else 1)
        if steps == 0 or nv == 0:
            return self.v.clone()
        xa = self.x.to(torch.float64).contiguous()
        if xa is self.x:
            xa = xa.clone()
        xb = torch.empty_like(xa)
        call('nksr_geom_smooth', ptr(xa), ptr(xb), nv, ptr(self.neighbour_start), ptr(self.neighbours), self.topology.edges.shape[0],
             ptr(self.neighbour_class), ptr(self.vertex_kind), ptr(mask), BOUNDARIES[boundary], steps, lam, mu if method == 'taubin' else lam,
             stream())
        return (xa if steps % 2 == 0 else xb).to(self.v.dtype)              # the one rounding
