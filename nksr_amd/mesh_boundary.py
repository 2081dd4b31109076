"""Triangle-mesh borders on the GPU: ``MeshBoundary`` (boundary edges ordered into loops, their measures, closing the small ones).

    b = MeshBoundary(v, f)                      # v numpy / torch fp32 / fp64 on any device, f int32 / int64 (float / bool faces refused)
    b = MeshBoundary.from_topology(t)           # reuse a MeshTopology: its edge table is the only set-up; b.topology is t
    r = b.loops()                               # ``BoundaryLoops`` (cached): loop_start, loop_vertices, loop_length, loop_area, ...
    keep = r.select(max_edges=50)               # [L] bool: closed (and simple) loops at or under every threshold given
    v2, f2, c2, new_vertex_mask, new_face_loop = b.fill(keep, method='centroid', colors=None)

Definition (kernels in csrc/meshbound.hip; restated in numpy by tests/mesh_boundary_ref.py):
  boundary    half-edge 3 f + k runs from corner k to corner k + 1 of a valid face.  The boundary half-edges are those whose unique edge
              has class NKSR_TOPO_BOUNDARY: B = topology.boundary_edges of them.  Boundary id b = the rank in ascending half-edge id
              (flags over [0, 3F), then an exclusive scan).  halfedge / tail / head / face [B].
  successor   rotation about the head: for the boundary half-edge (a -> b) of face f look at the next half-edge of f, (b -> c).  Its
              edge BOUNDARY: that half-edge is the successor.  INTERIOR: cross to face_adjacency[f, k + 1], find there the corner that
              holds (c -> b), take the half-edge after it, (b -> d), and repeat.  MISORIENTED or NONMANIFOLD: no successor (-1), the
              border is open there.  The walk needs no guard: incoming -> twin(next(incoming)) is injective on the half-edges that run
              into b, and a boundary half-edge has no pre-image under it, so the orbit is a simple path of at most valence(b) steps.
              succ is injective; pred, found by the mirrored walk about the tail, is its inverse.  The walk stays inside one fan of
              faces about b: two borders that touch in a vertex where each has a fan of its own (two bodies welded in a corner) come
              out as two loops, not as a figure-eight.  Where the surface itself is pinched (two fans, and a border on either side of
              each: a pinched disc, or two holes that meet corner to corner) each fan leads from one side to the other and the
              border is ONE loop that passes the vertex twice (loop_simple is false); connectivity alone cannot tell those apart.
              On an edge-manifold, consistently oriented mesh every boundary half-edge has a successor, so every loop is closed.
  loops       the cycles and maximal chains of succ (``chain_rank(pred)``, the list ranking of the slicer).  Representative: a cycle's
              smallest boundary id, an open chain's first element; rank = the succ steps from it; loop ids ascend by representative.
              loop_vertices = the tails in rank order, plus the last head of an open chain (m + 1 for m edges; a cycle has m);
              loop_start [L + 1] indexes it, loop_edge_start [L + 1] indexes loop_halfedges (m per loop).  loop_simple: no vertex is
              the tail of two half-edges of the loop (one sort of (loop, tail) keys and the shared run table).
  measures    all fp64, p_0 the representative's tail, p_i / p_i+1 tail and head of the half-edge of rank i, a = p_i - p_0,
              c = p_i+1 - p_0, positions read in the caller's precision (fp32 widened exactly), no recentring, every operation rounded
              on its own.  loop_length = sum w_i, w_i = sqrt(dx dx + dy dy + dz dz) of p_i+1 - p_i.  loop_area_vector = sum 0.5 (a x c),
              0 for an open chain; loop_area its norm.  loop_centroid = p_0 + (sum w_i 0.5 (a + c)) / sum w_i (the length-weighted mean
              of the edge midpoints), p_0 when sum w = 0.  loop_box [L, 6] = min xyz, max xyz.  The sums are by-key scans in rank
              order (nksr_inclusive_sum_by_key_f64).
  selection   ``select`` never includes an open chain.  The rim of an open surface is a loop like any other: a threshold (max_edges,
              max_length, max_area) is what tells it from a hole.
  fill        old vertices and faces keep their indices and dtypes; new faces are appended loop by loop in rank order.  'centroid': one
              new vertex per kept loop, V + its rank among the kept loops, at loop_centroid cast to the dtype of v once; for every
              boundary half-edge (a -> b) the face (b, a, c): m faces.  'fan': no new vertex; faces (p_i+1, p_i, p_0), i = 1 .. m - 2:
              m - 2 faces; a kept loop that is not simple raises ValueError.  Both wind the new faces against the boundary half-edges,
              so the new edges are INTERIOR and the orientation is preserved.  c2 of a new vertex = the fp64 mean of the loop's vertex
              colours in rank order, cast back.  The patch is flat; fairing it is
              ``MeshGeometry(v2, f2).smooth(..., fixed=~new_vertex_mask)`` ('centroid': only the new vertices move).
Every array repeats bit for bit: no floating-point atomic, ids are scans plus offsets, every write has one writer; the one atomic is the
integer min / max of the boxes.  ``loops`` synchronises once (L and the run count, B is the topology's), ``fill`` once (its sizes); the
half-edge -> edge map is ``MeshTopology.halfedge_edge``.  Limits: as MeshTopology; V + kept loops < 2^31 with int32 faces.
"""
import numbers

import torch

from . import ops
from ._lib import call, lib, ptr, stream
from .mesh_input import is64
from .mesh_slice import _run_totals, _sum_by_key, chain_rank
from .mesh_topology import MeshTopology

LIMIT = 1 << 31
STAGES = ('boundary', 'successor', 'rank', 'loops', 'simple', 'measures')       # 'rank' ends with the size read
FILL_STAGES = ('sizes', 'faces', 'vertices')                                     # 'sizes' ends with the size read
METHODS = {'centroid': 0, 'fan': 1}


def _f64(x):
    return int(x.dtype == torch.float64)


# ---- stages (nksr_amd/tools/prof_mesh_boundary.py times them one by one) -------------------------------------------------------------
def boundary_halfedges(f, he_edge, edge_classes, n_boundary):
    """(boundary_of [3F + 1] int32: the boundary id of a flagged half-edge, halfedge, tail, head, face [B] int32)."""
    nf, dev = f.shape[0], f.device
    flags = torch.empty(3 * nf + 1, dtype=torch.int32, device=dev)
    call('nksr_bnd_flags', ptr(he_edge), ptr(edge_classes), nf, edge_classes.shape[0], ptr(flags), stream())
    bid = ops.exclusive_sum_i32(flags)
    he, tail, head, face = (torch.empty(n_boundary, dtype=torch.int32, device=dev) for _ in range(4))
    call('nksr_bnd_list', ptr(f), is64(f), nf, ptr(flags), ptr(bid), n_boundary, ptr(he), ptr(tail), ptr(head), ptr(face), stream())
    return bid, he, tail, head, face


def successors(f, he_edge, edge_classes, face_adjacency, bid, halfedge):
    """(succ [B], pred [B]) int32, -1: none."""
    nb, dev = halfedge.shape[0], f.device
    succ = torch.empty(nb, dtype=torch.int32, device=dev)
    pred = torch.empty(nb, dtype=torch.int32, device=dev)
    call('nksr_bnd_successor', ptr(f), is64(f), f.shape[0], ptr(he_edge), ptr(edge_classes), ptr(face_adjacency), ptr(bid), ptr(halfedge), nb,
         ptr(succ), ptr(pred), stream())
    return succ, pred


def tail_runs(rep, tail):
    """The sorted (representative, tail) keys of the boundary half-edges and the block offsets of their run table, whose last entry is
    the number of distinct (loop, tail) pairs; nothing is read here."""
    nb, dev = rep.shape[0], rep.device
    keys = ops.sort_keys((rep.to(torch.int64) << 32) | tail.to(torch.int64), end_bit=32 + max(int(nb).bit_length(), 1))
    nblk = int(lib.nksr_run_blocks(nb))
    counts = torch.empty(nblk + 1, dtype=torch.int64, device=dev)
    call('nksr_run_counts_u64', ptr(keys), nb, 0xFFFFFFFFFFFFFFFF, ptr(counts), stream())
    return keys, ops.exclusive_sum_i64(counts)


def loop_sizes(rep, rank, cyclic, succ, dense, n_loops):
    """(boundary_loop [B], loop_rep [L], loop_edges [L + 1], loop_points [L + 1] int32 with a closing 0, closed [L] uint8)."""
    nb, dev = rep.shape[0], rep.device
    loop_of = torch.empty(nb, dtype=torch.int32, device=dev)
    loop_rep = torch.empty(n_loops, dtype=torch.int32, device=dev)
    n_edges = torch.empty(n_loops + 1, dtype=torch.int32, device=dev)
    n_pts = torch.empty(n_loops + 1, dtype=torch.int32, device=dev)
    closed = torch.empty(n_loops, dtype=torch.uint8, device=dev)
    call('nksr_bnd_loop_sizes', ptr(rep), ptr(rank), ptr(cyclic), ptr(succ), nb, ptr(dense), n_loops, ptr(loop_of), ptr(loop_rep), ptr(n_edges),
         ptr(n_pts), ptr(closed), stream())
    return loop_of, loop_rep, n_edges, n_pts, closed


def simple_loops(keys, offsets, n_runs, edge_start, loop_edges):
    """[L] bool: the loop has as many distinct tails as half-edges.  The keys are sorted by (loop, tail), so loop l owns the sorted
    positions [edge_start[l], edge_start[l + 1]) and its runs are those between the runs of its first and of its last position."""
    nb, dev = keys.shape[0], keys.device
    if loop_edges.shape[0] == 0:
        return torch.zeros(0, dtype=torch.bool, device=dev)
    start = torch.empty(n_runs + 1, dtype=torch.int32, device=dev)
    run_of = torch.empty(nb, dtype=torch.int32, device=dev)
    call('nksr_run_table_u64', ptr(keys), nb, 0xFFFFFFFFFFFFFFFF, ptr(offsets), n_runs, ptr(start), None, ptr(run_of), stream())
    first, last = edge_start[:-1].long(), edge_start[1:].long() - 1
    return (run_of[last] - run_of[first] + 1) == loop_edges


def loop_terms(x, halfedge, tail, head, rank, cyclic, succ, loop_of, loop_rep, edge_start, loop_start, n_points):
    """(loop_halfedges [B], loop_vertices [n_points] int32, term_key [B] int64, terms [7, B] fp64 in rank order)."""
    nb, nl, dev = halfedge.shape[0], loop_rep.shape[0], halfedge.device
    loop_he = torch.empty(nb, dtype=torch.int32, device=dev)
    loop_v = torch.empty(n_points, dtype=torch.int32, device=dev)
    key = torch.empty(nb, dtype=torch.int64, device=dev)
    terms = torch.empty((7, nb), dtype=torch.float64, device=dev)
    call('nksr_bnd_terms', ptr(x), _f64(x), x.shape[0], ptr(halfedge), ptr(tail), ptr(head), ptr(rank), ptr(cyclic), ptr(succ), nb, ptr(loop_of),
         ptr(loop_rep), ptr(edge_start), ptr(loop_start), nl, ptr(loop_he), ptr(loop_v), ptr(key), ptr(terms), stream())
    return loop_he, loop_v, key, terms


def loop_boxes(x, tail, head, loop_of, n_loops):
    dev = x.device
    box = torch.empty((n_loops, 6), dtype=torch.float64, device=dev)
    work = torch.empty((n_loops, 6), dtype=torch.int64, device=dev)
    call('nksr_bnd_boxes', ptr(x), _f64(x), x.shape[0], ptr(tail), ptr(head), ptr(loop_of), tail.shape[0], n_loops, ptr(work), ptr(box), stream())
    return box


class BoundaryLoops:
    """The result of ``MeshBoundary.loops``: device tensors, integers int32 unless noted.  n_boundary B, n_loops L.
    halfedge / tail / head / face [B] in ascending half-edge id; succ / pred [B] (-1: none); boundary_loop / boundary_rank [B];
    loop_start [L + 1] into loop_vertices (m + 1 entries for an open chain of m edges), loop_edge_start [L + 1] into loop_halfedges;
    loop_rep [L] (the representative boundary id), loop_edges [L], loop_closed / loop_simple [L] bool; loop_length / loop_area [L],
    loop_area_vector / loop_centroid [L, 3], loop_box [L, 6] fp64; rounds = the ranking rounds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def select(self, max_edges=None, max_length=None, max_area=None, simple_only=True):
        """[L] bool: the closed loops with at most ``max_edges`` edges, a length of at most ``max_length`` and an area of at most
        ``max_area`` (None: no limit), the simple ones only unless ``simple_only=False``.  An open chain is never selected.  The rim
        of an open surface is a loop like any other: a threshold is what tells it from a hole."""
        for name, x in (('max_edges', max_edges), ('max_length', max_length), ('max_area', max_area)):
            if x is not None and (isinstance(x, bool) or not isinstance(x, numbers.Real) or x != x or x < 0):
                raise ValueError('select: %s must be a non-negative number or None, got %r' % (name, x))
        keep = self.loop_closed.clone()
        if simple_only:
            keep &= self.loop_simple
        if max_edges is not None:
            keep &= self.loop_edges <= max_edges
        if max_length is not None:
            keep &= self.loop_length <= float(max_length)
        if max_area is not None:
            keep &= self.loop_area <= float(max_area)
        return keep


class MeshBoundary:
    """The borders of one triangle mesh (v [V, 3], f [F, 3] int32 / int64) on the GPU; see the module's docstring."""

    def __init__(self, v, f, device=None):
        self._init(MeshTopology(v, f, device))

    @classmethod
    def from_topology(cls, topology):
        """The boundary loops over the edge table of a ``MeshTopology`` that exists already."""
        if not isinstance(topology, MeshTopology):
            raise TypeError('from_topology: expected a MeshTopology, got %s' % type(topology).__name__)
        b = cls.__new__(cls)
        b._init(topology)
        return b

    def _init(self, t):
        self.topology, self.device = t, t.device
        self.v, self.f = t.v, t.f
        self.x = t.v if t.v.dtype in (torch.float32, torch.float64) else t.v32        # what the kernels read
        self.n_vertices, self.n_faces = t.n_vertices, t.n_faces
        self._loops = None

    def loops(self, _mark=None):
        """``BoundaryLoops`` of this mesh, computed on the first call and kept.  (``_mark(stage)`` is called after every stage of
        STAGES: the profiler's hook; with it the result is computed afresh.)"""
        if self._loops is not None and _mark is None:
            return self._loops
        mark = _mark or (lambda stage: None)
        t, dev, x = self.topology, self.device, self.x
        nb = int(t.boundary_edges)
        bid, he, tail, head, face = boundary_halfedges(self.f, t.halfedge_edge, t.edge_classes, nb)
        mark('boundary')
        succ, pred = successors(self.f, t.halfedge_edge, t.edge_classes, t.face_adjacency, bid, he)
        mark('successor')
        rep, rank, cyclic, flags = chain_rank(pred)
        dense = ops.exclusive_sum_i32(flags)
        keys, run_offsets = tail_runs(rep, tail)
        n_open = ((flags[:nb] != 0) & (cyclic == 0)).sum()
        nl, n_open, n_runs = (int(c) for c in torch.stack([dense[nb].long(), n_open, run_offsets[-1]]).tolist())      # the sync: L
        mark('rank')
        loop_of, loop_rep, n_edges, n_pts, closed = loop_sizes(rep, rank, cyclic, succ, dense, nl)
        edge_start, loop_start = ops.exclusive_sum_i32(n_edges), ops.exclusive_sum_i32(n_pts)
        loop_he, loop_v, key, terms = loop_terms(x, he, tail, head, rank, cyclic, succ, loop_of, loop_rep, edge_start, loop_start, nb + n_open)
        mark('loops')
        simple = simple_loops(keys, run_offsets, n_runs, edge_start, n_edges[:nl])
        mark('simple')
        end = edge_start[1:]
        sums = [_run_totals(_sum_by_key(key, terms[k]), end) for k in range(7)]
        length = sums[0]
        area_vector = torch.stack(sums[1:4], 1) if nl else torch.zeros((0, 3), dtype=torch.float64, device=dev)
        area = torch.sqrt(area_vector[:, 0] * area_vector[:, 0] + area_vector[:, 1] * area_vector[:, 1] + area_vector[:, 2] * area_vector[:, 2])
        p0 = x[tail[loop_rep.long()].long()].to(torch.float64).reshape(-1, 3)
        moment = torch.stack(sums[4:7], 1) if nl else torch.zeros((0, 3), dtype=torch.float64, device=dev)
        centroid = torch.where((length > 0)[:, None], p0 + moment / length[:, None], p0)
        box = loop_boxes(x, tail, head, loop_of, nl)
        mark('measures')
        r = BoundaryLoops(n_boundary=nb, n_loops=nl, rounds=int(lib.nksr_chain_rank_rounds(nb)) if nb else 0, halfedge=he, tail=tail, head=head,
                          face=face, succ=succ, pred=pred, boundary_loop=loop_of, boundary_rank=rank, loop_start=loop_start,
                          loop_edge_start=edge_start, loop_halfedges=loop_he, loop_vertices=loop_v, loop_rep=loop_rep,
                          loop_edges=n_edges[:nl].contiguous(), loop_closed=closed.bool(), loop_simple=simple, loop_length=length,
                          loop_area_vector=area_vector, loop_area=area, loop_centroid=centroid, loop_box=box)
        if _mark is None:
            self._loops = r
        return r

    def fill(self, keep, method='centroid', colors=None, _mark=None):
        """(v2, f2, c2, new_vertex_mask [V2] bool, new_face_loop [F2 - F] int32): the mesh with the loops flagged in ``keep`` [L]
        (``BoundaryLoops.select``) closed.  Old vertices and faces keep their indices and dtypes; the new faces follow, loop by loop
        in rank order.  'centroid': one new vertex per kept loop at ``loop_centroid`` and one face per boundary half-edge.  'fan': no
        new vertex, faces (p_i+1, p_i, p_0); a kept loop that is not simple raises ValueError.  An open chain in ``keep`` raises
        ValueError.  ``c2``: ``colors`` [V, C] with, under 'centroid', the fp64 mean of the loop's vertex colours per new vertex, cast
        back (None without colours).  The patch is flat: fair it with ``MeshGeometry(v2, f2).smooth(..., fixed=~new_vertex_mask)``."""
        if method not in METHODS:
            raise ValueError("method must be 'centroid' or 'fan', got %r" % (method,))
        mark = _mark or (lambda stage: None)
        r, dev, nv, nf = self.loops(), self.device, self.n_vertices, self.n_faces
        keep = torch.as_tensor(keep).to(dev)
        if keep.shape != (r.n_loops,):
            raise ValueError('fill: expected %d loop flags, got shape %s' % (r.n_loops, tuple(keep.shape)))
        keep = keep != 0
        if colors is not None:
            colors = torch.as_tensor(colors).to(dev)
            if colors.ndim != 2 or colors.shape[0] != nv:
                raise ValueError('fill: expected [%d, C] colours, got shape %s' % (nv, tuple(colors.shape)))
        centroid = method == 'centroid'
        per_loop = torch.where(keep, r.loop_edges if centroid else (r.loop_edges - 2).clamp(min=0), torch.zeros_like(r.loop_edges))
        counts = torch.cat([per_loop, per_loop.new_zeros(1)])
        kept = torch.cat([keep.to(torch.int32), per_loop.new_zeros(1)])
        face_offset, kept_rank = ops.exclusive_sum_i32(counts), ops.exclusive_sum_i32(kept)
        n_new, n_kept, n_open, n_knot = (int(c) for c in torch.stack([face_offset[-1].long(), kept_rank[-1].long(), (keep & ~r.loop_closed).sum(),
                                                                     (keep & ~r.loop_simple).sum()]).tolist())       # the sync: the fill sizes
        if n_open:
            raise ValueError('fill: %d of the kept loops are open chains, which cannot be closed' % n_open)
        if not centroid and n_knot:
            raise ValueError("fill: %d of the kept loops pass a vertex twice; method='fan' needs simple loops (use 'centroid')" % n_knot)
        n_added = n_kept if centroid else 0
        if not is64(self.f) and nv + n_added >= LIMIT:
            raise ValueError('fill: %d vertices and %d new ones, at most 2^31 - 1 with int32 faces' % (nv, n_added))
        mark('sizes')
        keep8 = keep.to(torch.uint8)
        f2 = torch.empty((nf + n_new, 3), dtype=self.f.dtype, device=dev)
        f2[:nf] = self.f
        new_faces = torch.empty((n_new, 3), dtype=self.f.dtype, device=dev)
        face_loop = torch.empty(n_new, dtype=torch.int32, device=dev)
        call('nksr_bnd_fill', ptr(r.tail), ptr(r.head), ptr(r.boundary_rank), ptr(r.boundary_loop), r.n_boundary, ptr(r.loop_rep), ptr(r.loop_edges),
             ptr(keep8), ptr(kept_rank), ptr(face_offset), r.n_loops, METHODS[method], nv, n_new, ptr(new_faces), is64(self.f), ptr(face_loop), stream())
        f2[nf:] = new_faces
        mark('faces')
        v2 = torch.empty((nv + n_added, 3), dtype=self.v.dtype, device=dev)
        v2[:nv] = self.v
        mask = torch.zeros(nv + n_added, dtype=torch.bool, device=dev)
        mask[nv:] = True
        c2 = colors
        if n_added:
            cx, channels = None, 0
            if colors is not None:
                cx = (colors if colors.dtype in (torch.float32, torch.float64) else colors.to(torch.float64)).contiguous()
                channels = int(cx.shape[1])
            new_v = torch.empty((n_added, 3), dtype=self.x.dtype, device=dev)
            mean = torch.empty((n_added, channels), dtype=torch.float64, device=dev) if channels else None
            call('nksr_bnd_fill_vertices', ptr(r.loop_centroid), ptr(r.loop_start), ptr(r.loop_vertices), ptr(r.loop_edges), ptr(keep8), ptr(kept_rank),
                 r.n_loops, n_added, ptr(cx) if channels else None, _f64(cx) if channels else 0, channels, nv, ptr(new_v), _f64(new_v), ptr(mean),
                 stream())
            v2[nv:] = new_v.to(self.v.dtype)
            if colors is not None:
                c2 = torch.cat([colors, (mean if channels else colors.new_zeros((n_added, 0))).to(colors.dtype)])
        mark('vertices')
        return v2, f2, c2, mask, face_loop
