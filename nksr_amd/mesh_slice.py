"""Triangle-mesh cross-sections on the GPU: ``MeshSlicer`` (plane slices and contours as ordered polylines).

    s = MeshSlicer(v, f)                        # v numpy / torch fp32 / fp64 on any device, f int32 / int64 (float / bool faces refused)
    s = MeshSlicer.from_topology(t)             # reuse a MeshTopology: its edge table is the only set-up; s.topology is t
    r = s.slice(normal, offsets)                # one family of parallel planes { x : n . x = offsets[j] }, n = normal / |normal|
    r = s.contours(levels=None, interval=None, axis=2)      # normal = +e_axis; interval: its multiples in (min h, max h]
    r.points, r.segments, r.polyline_start, r.polyline_points, r.polyline_length, r.polyline_area, r.plane_area, ...    # ``Sections``

Definition (kernels in csrc/meshslice.hip; restated in numpy by tests/mesh_slice_ref.py):
  heights     h_v = fma(n_z, z, fma(n_y, y, n_x x)) in fp64, positions read in the caller's precision (fp32 widened exactly), no
              recentring.  Vertex v is ABOVE plane j iff h_v >= o_j: a vertex exactly on a plane counts as above.  (A height that is
              not a number is stored as -inf: below every plane.)
  crossings   a valid face crosses plane j iff min h < o_j <= max h over its corners: the planes [lo_f, hi_f) of the sorted offsets.
              It then has exactly one half-edge going above -> below and one going below -> above.  Invalid faces cross nothing.
  points      one per (unique edge e = (a, b), a < b, plane j) with o_j in (min(h_a, h_b), max(h_a, h_b)]; id = point_start[e] + (j - lo_e),
              point_start the exclusive scan of the edges' counts.  p = a + t (b - a), t = (o_j - h_a) / (h_b - h_a) in fp64, every
              operation rounded on its own, always from the canonical end points: both faces of an edge see the same bits.  A vertex
              exactly on a plane yields coincident points on its crossing edges and zero-length segments between them.
  segments    one per (face, crossed plane); id = seg_start[f] + (j - lo_f): face-major, the plane ascending within a face.  tail = the
              point on the above -> below half-edge, head = the point on the below -> above one: the direction is n x n_face, so with
              outward normals loops run counter-clockwise seen from the tip of n and holes clockwise.
  successor   succ[s] = the segment of the same plane in the face across the half-edge that carries head(s), iff that edge's class is
              NKSR_TOPO_INTERIOR; boundary, misoriented and non-manifold edges end a polyline.  No segment is ever dropped.
  polylines   the maximal chains and the cycles of succ.  Representative: an open chain's segment without predecessor, a cycle's
              smallest segment id; rank = the succ steps from it.  Polyline ids ascend by (plane, representative).  polyline_points =
              the tails in rank order, plus the last head of an open chain (m + 1 points for m segments; a cycle has m).
  measures    segment length sqrt(dx dx + dy dy + dz dz); polyline_length = their sum in rank order; polyline_area =
              sum of 0.5 n . ((p_i - p_0) x (p_i+1 - p_0)) over a cycle in rank order, p_0 the representative's tail, 0 for an open
              polyline; plane totals are sums in polyline order.  All sums are by-key scans (nksr_inclusive_sum_by_key_f64).
Every array repeats bit for bit: there is no atomic of any kind, ids are scans plus offsets and every write has one writer.  The ordering
of the segments is list ranking by pointer doubling (``chain_rank``, generic over any predecessor array): ceil(log2 S) + 1 rounds queued
without a host read between them.  ``slice`` synchronises twice: to read N and S, then L.  Limits: as MeshTopology, and N, S,
S + L < 2^31.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import mesh_topology, ops
from ._lib import call, lib, ptr, stream, with_tmp
from .mesh_input import is64
from .mesh_topology import MeshTopology

LIMIT = 1 << 31
STAGES = ('heights', 'counts', 'points', 'segments', 'rank', 'polylines', 'measures')        # 'counts' and 'rank' end with the size reads
POINTS_BY_POINT = 0         # nksr_slice_points: one lane per edge, the faster shape at every size measured (profiles/mesh_slice.md); 1: one lane per point


def _normal3(normal):
    return (C.c_double * 3)(*[float(x) for x in normal])


# ---- stages (nksr_amd/tools/prof_mesh_slice.py times them one by one) ---------------------------------------------------------------
def halfedge_edges(keys_sorted, ids_sorted, nv):
    """[3F] int32: the unique edge of every half-edge 3 f + k (-1 for an invalid face); ``mesh_topology.halfedge_edges``, which
    ``MeshTopology.halfedge_edge`` computes once for the slicer and the boundary loops alike."""
    return mesh_topology.halfedge_edges(keys_sorted, ids_sorted, nv)


def heights(x, normal):
    """[V] fp64 heights along the unit ``normal`` (three floats)."""
    h = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    call('nksr_slice_heights', ptr(x), int(x.dtype == torch.float64), x.shape[0], _normal3(normal), ptr(h), stream())
    return h


def plane_ranges(h, f, face_valid, edges, offsets):
    """(lo_f [F] int32, seg_start [F + 1] int64, lo_e [E] int32, point_start [E + 1] int64): the counts and their exclusive scans."""
    nf, ne, dev = f.shape[0], edges.shape[0], f.device
    lo_f = torch.empty(nf, dtype=torch.int32, device=dev)
    cnt_f = torch.empty(nf + 1, dtype=torch.int64, device=dev)
    lo_e = torch.empty(ne, dtype=torch.int32, device=dev)
    cnt_e = torch.empty(ne + 1, dtype=torch.int64, device=dev)
    call('nksr_slice_counts', ptr(h), h.shape[0], ptr(f), is64(f), nf, ptr(face_valid), ptr(edges), ne, ptr(offsets), offsets.shape[0], ptr(lo_f),
         ptr(cnt_f), ptr(lo_e), ptr(cnt_e), stream())
    return lo_f, ops.exclusive_sum_i64(cnt_f), lo_e, ops.exclusive_sum_i64(cnt_e)


def edge_points(x, h, edges, offsets, lo_e, point_start, n, by_point=POINTS_BY_POINT):
    """(points [N, 3] fp64, point_edge [N], point_plane [N] int32)."""
    dev = x.device
    points = torch.empty((n, 3), dtype=torch.float64, device=dev)
    point_edge = torch.empty(n, dtype=torch.int32, device=dev)
    point_plane = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_slice_points', ptr(x), int(x.dtype == torch.float64), x.shape[0], ptr(h), ptr(edges), edges.shape[0], ptr(offsets), offsets.shape[0],
         ptr(lo_e), ptr(point_start), n, int(by_point), ptr(points), ptr(point_edge), ptr(point_plane), stream())
    return points, point_edge, point_plane


def face_segments(h, f, offsets, he_edge, edge_classes, face_adjacency, lo_f, seg_start, lo_e, point_start, n):
    """(segments [S, 2], segment_face [S], segment_plane [S], succ [S], pred [S]) int32."""
    dev = f.device
    seg = torch.empty((n, 2), dtype=torch.int32, device=dev)
    face, plane, succ, pred = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    call('nksr_slice_segments', ptr(h), h.shape[0], ptr(f), is64(f), f.shape[0], ptr(offsets), offsets.shape[0], ptr(he_edge), ptr(edge_classes),
         ptr(face_adjacency), ptr(lo_f), ptr(seg_start), ptr(lo_e), ptr(point_start), n, ptr(seg), ptr(face), ptr(plane), ptr(succ), ptr(pred), stream())
    return seg, face, plane, succ, pred


def chain_rank(pred):
    """List ranking of the chains and cycles of a predecessor array [n] int32 (-1: none; the inverse of an injective successor array):
    (rep [n], rank [n] int32, cyclic [n] uint8, rep_flags [n + 1] int32).  rep = the element without predecessor of an open chain, the
    smallest element of a cycle; rank = the steps from it.  ``chain_rank_rounds(n)`` doubling rounds, no host read."""
    n, dev = pred.shape[0], pred.device
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    cyclic = torch.empty(n, dtype=torch.uint8, device=dev)
    flags = torch.empty(n + 1, dtype=torch.int32, device=dev)
    work = torch.empty((2 * n, 4), dtype=torch.int32, device=dev)
    call('nksr_chain_rank', ptr(pred), n, ptr(work), ptr(rep), ptr(rank), ptr(cyclic), ptr(flags), stream())
    return rep, rank, cyclic, flags


def chain_rank_rounds(n):
    return int(lib.nksr_chain_rank_rounds(int(n)))


def _sum_by_key(keys, terms):
    out = torch.empty_like(terms)
    if terms.numel():
        with_tmp('nksr_inclusive_sum_by_key_f64', terms.device, ptr(keys), ptr(terms), ptr(out), terms.numel(), stream())
    return out


def _run_totals(sums, end, dtype=torch.float64):
    """The last entry of every run of an inclusive by-key sum: ``end`` [R] = one past the run's last position; 0 for an empty run."""
    n = sums.shape[0]
    if n == 0:
        return torch.zeros(end.shape[0], dtype=dtype, device=end.device)
    first = torch.cat([end.new_zeros(1), end])[:-1]
    return torch.where(end > first, sums[(end - 1).clamp(min=0).long()], sums.new_zeros(()))


class Sections:
    """The result of ``MeshSlicer.slice``: device tensors, integers int32 unless noted.  n_points N, n_segments S, n_polylines L, n_planes P.
    normal (three floats, unit), offsets [P] fp64; vertex_height [V] fp64; points64 [N, 3] fp64 (``points``: the dtype of v),
    point_edge / point_plane [N]; segments [S, 2] (tail, head), segment_face / segment_plane [S], succ / pred [S] (-1: none),
    segment_polyline / segment_rank [S]; polyline_start [L + 1] into polyline_points; polyline_rep [L] (the representative segment),
    polyline_closed [L] bool, polyline_plane [L], polyline_length / polyline_area [L] fp64; plane_length / plane_area [P] fp64,
    plane_open [P] (open polylines: when > 0 the area is no cross-section area), plane_polyline_start [P + 1]; rounds = the ranking rounds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def points(self):
        return self.points64.to(self.dtype)

    def polylines_of(self, j):
        """The ``slice`` of polyline ids of plane j (one host read)."""
        if not 0 <= int(j) < self.n_planes:
            raise IndexError('plane %r of %d' % (j, self.n_planes))
        a, b = self.plane_polyline_start[int(j):int(j) + 2].tolist()
        return slice(a, b)


class MeshSlicer:
    """Cross-sections of one triangle mesh (v [V, 3], f [F, 3] int32 / int64) on the GPU; see the module's docstring."""

    def __init__(self, v, f, device=None):
        self._init(MeshTopology(v, f, device))

    @classmethod
    def from_topology(cls, topology):
        """The slicer over the edge table of a ``MeshTopology`` that exists already."""
        if not isinstance(topology, MeshTopology):
            raise TypeError('from_topology: expected a MeshTopology, got %s' % type(topology).__name__)
        s = cls.__new__(cls)
        s._init(topology)
        return s

    def _init(self, t):
        self.topology, self.device = t, t.device
        self.v, self.f = t.v, t.f
        self.x = t.v if t.v.dtype in (torch.float32, torch.float64) else t.v32        # what the kernels read
        self.n_vertices, self.n_faces = t.n_vertices, t.n_faces
        self.halfedge_edge = t.halfedge_edge

    # ---- arguments ----
    @staticmethod
    def _unit(normal):
        try:
            n = np.asarray(normal, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError('normal: expected three numbers, got %r' % (normal,))
        if n.shape != (3,) or not np.all(np.isfinite(n)):
            raise ValueError('normal: expected three finite numbers, got %r' % (normal,))
        scale = float(np.max(np.abs(n)))
        if scale == 0.0:
            raise ValueError('normal: the zero vector has no direction')
        n = n / scale                                   # (no overflow or underflow in the norm)
        n = n / math.sqrt(float(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]))
        return [float(x) for x in n]

    def _offsets(self, offsets):
        if isinstance(offsets, torch.Tensor):
            offsets = offsets.detach().cpu().numpy()
        try:
            o = np.asarray(offsets, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('offsets: expected a 1-D array of numbers')
        if o.ndim != 1:
            raise ValueError('offsets: expected a 1-D array, got shape %s' % (o.shape,))
        if o.shape[0] >= LIMIT:
            raise ValueError('offsets: %d planes, at most 2^31 - 1' % o.shape[0])
        if not np.all(np.isfinite(o)):
            raise ValueError('offsets: non-finite values')
        if o.shape[0] > 1 and not np.all(o[1:] > o[:-1]):
            raise ValueError('offsets: must be strictly increasing')
        return torch.from_numpy(np.ascontiguousarray(o)).to(self.device)

    # ---- the passes ----
    def slice(self, normal, offsets, _mark=None):
        """``Sections`` of the planes { x : n . x = offsets[j] }, n = normal / |normal| (normalised in fp64 on the host); ``offsets`` a
        1-D array of finite, strictly increasing values (else ValueError), possibly empty.  Planes of another normal: another call.
        (``_mark(stage)`` is called after every stage of STAGES: the profiler's hook.)"""
        mark = _mark or (lambda stage: None)
        n3 = self._unit(normal)
        off = self._offsets(offsets)
        t, dev = self.topology, self.device
        nplanes = int(off.shape[0])
        h = heights(self.x, n3)
        mark('heights')
        lo_f, seg_start, lo_e, point_start = plane_ranges(h, self.f, t.face_valid, t.edges, off)
        npts, nseg = (int(c) for c in torch.stack([point_start[-1], seg_start[-1]]).tolist())       # sync 1: N and S
        if npts >= LIMIT or nseg >= LIMIT:
            raise ValueError('mesh slicer: %d points and %d segments, at most 2^31 - 1 each' % (npts, nseg))
        mark('counts')
        points, point_edge, point_plane = edge_points(self.x, h, t.edges, off, lo_e, point_start, npts)
        mark('points')
        seg, seg_face, seg_plane, succ, pred = face_segments(h, self.f, off, self.halfedge_edge, t.edge_classes, t.face_adjacency, lo_f, seg_start,
                                                             lo_e, point_start, nseg)
        mark('segments')
        rep, rank, cyclic, flags = chain_rank(pred)
        dense = ops.exclusive_sum_i32(flags)
        n_open = (flags[:nseg] != 0) & (cyclic == 0)                                                # (an open chain's first segment)
        npoly, n_open = (int(c) for c in torch.stack([dense[nseg].long(), n_open.sum()]).tolist())  # sync 2: L (and the open ones among them)
        if nseg + npoly >= LIMIT:
            raise ValueError('mesh slicer: %d segments in %d polylines, their sum at most 2^31 - 1' % (nseg, npoly))
        mark('rank')
        rep_list = torch.empty(npoly, dtype=torch.int32, device=dev)
        plane_key = torch.empty(npoly, dtype=torch.int64, device=dev)
        call('nksr_slice_rep_list', ptr(flags), ptr(dense), nseg, ptr(seg_plane), npoly, ptr(rep_list), ptr(plane_key), stream())
        # polyline ids ascend by (plane, representative): a stable sort by plane of the representatives, which ascend already
        poly_plane, order = ops.sort_pairs(plane_key, torch.arange(npoly, dtype=torch.int32, device=dev), end_bit=max(nplanes.bit_length(), 1))
        poly_rep = rep_list[order.long()]
        poly_of_dense = torch.empty(npoly, dtype=torch.int32, device=dev)
        poly_of_dense[order.long()] = torch.arange(npoly, dtype=torch.int32, device=dev)
        seg_poly = torch.empty(nseg, dtype=torch.int32, device=dev)
        n_segs = torch.empty(npoly + 1, dtype=torch.int32, device=dev)
        n_pts = torch.empty(npoly + 1, dtype=torch.int32, device=dev)
        closed = torch.empty(npoly, dtype=torch.uint8, device=dev)
        call('nksr_slice_polyline_sizes', ptr(rep), ptr(rank), ptr(cyclic), ptr(succ), nseg, ptr(dense), ptr(poly_of_dense), npoly, ptr(seg_poly),
             ptr(n_segs), ptr(n_pts), ptr(closed), stream())
        seg_offset, polyline_start = ops.exclusive_sum_i32(n_segs), ops.exclusive_sum_i32(n_pts)
        closed = closed.bool()
        poly_points = torch.empty(nseg + n_open, dtype=torch.int32, device=dev)     # (an open polyline has one point more than segments)
        term_key = torch.empty(nseg, dtype=torch.int64, device=dev)
        len_term = torch.empty(nseg, dtype=torch.float64, device=dev)
        area_term = torch.empty(nseg, dtype=torch.float64, device=dev)
        call('nksr_slice_polylines', ptr(seg), ptr(rank), ptr(cyclic), ptr(succ), nseg, ptr(seg_poly), ptr(poly_rep), ptr(seg_offset), ptr(polyline_start),
             npoly, ptr(points), npts, _normal3(n3), ptr(poly_points), ptr(term_key), ptr(len_term), ptr(area_term), stream())
        mark('polylines')
        seg_end = seg_offset[1:]
        poly_length = _run_totals(_sum_by_key(term_key, len_term), seg_end)
        poly_area = _run_totals(_sum_by_key(term_key, area_term), seg_end)
        # plane totals: the polylines of plane j are [plane_polyline_start[j], plane_polyline_start[j + 1])
        plane_poly_start = torch.searchsorted(poly_plane, torch.arange(nplanes + 1, dtype=torch.int64, device=dev)).to(torch.int32)
        plane_end = plane_poly_start[1:]
        plane_length = _run_totals(_sum_by_key(poly_plane, poly_length), plane_end)
        plane_area = _run_totals(_sum_by_key(poly_plane, poly_area), plane_end)
        open_before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((~closed).to(torch.int64), 0)])
        plane_open = (open_before[plane_end.long()] - open_before[plane_poly_start[:-1].long()]).to(torch.int32)
        mark('measures')
        return Sections(normal=n3, offsets=off, dtype=self.v.dtype if self.v.dtype.is_floating_point else torch.float32, n_planes=nplanes,
                        n_points=npts, n_segments=nseg, n_polylines=npoly, rounds=chain_rank_rounds(nseg) if nseg else 0,
                        vertex_height=h, points64=points, point_edge=point_edge, point_plane=point_plane, point_start=point_start,
                        segments=seg, segment_face=seg_face, segment_plane=seg_plane, seg_start=seg_start, succ=succ, pred=pred,
                        segment_polyline=seg_poly, segment_rank=rank, polyline_start=polyline_start, polyline_points=poly_points,
                        polyline_rep=poly_rep, polyline_closed=closed, polyline_plane=poly_plane.to(torch.int32), polyline_length=poly_length,
                        polyline_area=poly_area, plane_length=plane_length, plane_area=plane_area, plane_open=plane_open,
                        plane_polyline_start=plane_poly_start)

    def interval_levels(self, interval, axis, origin=0.0):
        """[n] fp64 numpy: the levels origin + k interval (k an integer) in (min, max] of the coordinate ``axis`` over the referenced
        vertices (two host reads); what ``contours(interval=)`` cuts at, and ``MeshClipper.tiles``."""
        try:
            step, origin = float(interval), float(origin)
        except (TypeError, ValueError):
            raise ValueError('interval must be a positive finite number, got %r' % (interval,))
        if not (step > 0.0 and math.isfinite(step) and math.isfinite(origin)):
            raise ValueError('interval must be a positive finite number, got %r' % (interval,))
        levels = np.zeros(0, np.float64)
        if self.topology.referenced_vertices:
            ref = self.topology.vertex_ref.bool()
            z = self.x[:, axis].to(torch.float64)
            lo = float(torch.where(ref, z, z.new_full((), math.inf)).amin().item())
            hi = float(torch.where(ref, z, z.new_full((), -math.inf)).amax().item())
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError('contours: non-finite coordinates along axis %d' % axis)
            k0, k1 = math.floor((lo - origin) / step) - 1, math.floor((hi - origin) / step) + 1
            if k1 - k0 > 1 << 24:
                raise ValueError('interval %r gives %d levels, at most 2^24' % (interval, k1 - k0))
            levels = np.arange(k0, k1 + 1, dtype=np.float64) * step
            if origin != 0.0:
                levels = origin + levels
            levels = levels[(levels > lo) & (levels <= hi)]
        return levels

    def contours(self, levels=None, interval=None, axis=2):
        """``slice`` with normal = +e_axis: at ``levels``, or at the multiples of ``interval`` in (min h, max h] over the referenced
        vertices (two more host reads).  Exactly one of the two."""
        if (levels is None) == (interval is None):
            raise ValueError('give exactly one of levels and interval')
        if isinstance(axis, bool) or axis not in (0, 1, 2):
            raise ValueError('axis must be 0, 1 or 2, got %r' % (axis,))
        normal = [0.0, 0.0, 0.0]
        normal[axis] = 1.0
        if levels is None:
            levels = self.interval_levels(interval, axis)
        return self.slice(normal, levels)
