"""Triangle-mesh topology on the GPU: ``MeshTopology`` (the unique-edge table, edge classes, connected components with their
statistics, removal of small components).

    t = MeshTopology(v, f)                     # v / f numpy or torch, f int32 / int64; builds the edge table once
    t.num_edges, t.boundary_edges, t.nonmanifold_edges, t.misoriented_edges, t.invalid_faces, t.referenced_vertices
    t.euler_characteristic                     # referenced V - E + valid F
    t.is_watertight                            # closed, edge-manifold and consistently oriented: MeshQuery.occupancy is exact
    c = t.components('edge')                   # or 'vertex': labels, counts, Euler characteristic, area and box per component
    keep = c.select(min_faces=10)              # [n] bool
    v2, f2, c2, vmap = t.compact(c.face_mask(keep), colors)

The edge table is the sorted list of the faces' half-edges cut into runs of equal (min, max) vertex pair (``ops.sorted_runs``, the run
table every sorted key list here shares; csrc/meshtopo.hip); components are a union-find over (face, face) pairs round every edge ('edge', the mesh notion) or over the edges as
(vertex, vertex) pairs ('vertex', the graph notion).  A face with an index outside [0, V) or with two equal indices is invalid: it has
no edges, label -1, is never kept, and is counted.  Every result repeats bit for bit: the roots of the union-find are the minimum node
index of each component whatever order the lanes ran in, the counts are integers, and the one floating-point sum (areas) is a scan in
a fixed order.  Limits: V < 2^31, F <= 2^30.  Input: nksr_amd/mesh_input.py (float and bool faces are refused).
"""
import numpy as np
import torch

from . import mesh_input, ops
from ._lib import (TOPO_BOUNDARY, TOPO_INTERIOR, TOPO_MAX_FACES, TOPO_MISORIENTED, TOPO_NONMANIFOLD, TOPO_TOTALS, call, lib, ptr, stream,  # noqa: F401
                   with_tmp)
from .mesh_input import gpu_device, is64, rows3

CONNECTIVITIES = ('edge', 'vertex')


# ---- stages (nksr_amd/tools/prof_mesh_topology.py times them one by one) --------------------------------------------------------------
def halfedge_keys(f, nv):
    """(keys [3F] int64, half-edge ids [3F] int32, face_valid [F] uint8, vertex_ref [V] uint8)."""
    nf, dev = f.shape[0], f.device
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    ids = torch.empty(3 * nf, dtype=torch.int32, device=dev)
    valid = torch.empty(nf, dtype=torch.uint8, device=dev)
    ref = torch.empty(nv, dtype=torch.uint8, device=dev)
    call('nksr_topo_halfedge_keys', ptr(f), is64(f), nf, nv, ptr(keys), ptr(ids), ptr(valid), ptr(ref), stream())
    return keys, ids, valid, ref


def sort_halfedges(keys, ids, nv):
    """One stable radix sort of the 32 + bit_length(V) key bits: half-edges of one edge stay in ascending id order."""
    return ops.sort_pairs(keys, ids, end_bit=32 + int(nv).bit_length())


class EdgeTable:
    """Device arrays of the unique-edge table and the totals read back from it."""


def edge_runs(f, nv, ks, ids_sorted, ref):
    """The runs of the sorted keys before the invalid faces' key -> edges, counts, classes, face adjacency, totals (syncs twice: E,
    then the totals)."""
    nf, dev = f.shape[0], f.device
    t = EdgeTable()
    ne, t.edge_start, edge_keys, _ = ops.sorted_runs(ks, none_from=(nv << 32) | nv, keys=True)
    t.edges = torch.empty((ne, 2), dtype=torch.int32, device=dev)
    t.edge_counts = torch.empty(ne, dtype=torch.int32, device=dev)
    t.edge_classes = torch.empty(ne, dtype=torch.uint8, device=dev)
    t.face_adjacency = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    totals = torch.empty(TOPO_TOTALS, dtype=torch.int64, device=dev)
    call('nksr_topo_edge_classes', ptr(f), is64(f), nf, nv, ptr(ids_sorted), ptr(edge_keys), ptr(t.edge_start), ne, ptr(ref), ptr(t.edges),
         ptr(t.edge_counts), ptr(t.edge_classes), ptr(t.face_adjacency), ptr(totals), stream())
    t.totals = [int(x) for x in totals.tolist()]
    return t


def halfedge_edges(keys_sorted, ids_sorted, nv):
    """[3F] int32: the unique edge of every half-edge 3 f + k (-1 for an invalid face): the run of its sorted key (``ops.sorted_runs``,
    the edge table's own runs) scattered through the sort's permutation.  Syncs once (the number of runs)."""
    _, _, _, run_of = ops.sorted_runs(keys_sorted, none_from=(nv << 32) | nv, run_of=True)
    he = torch.empty_like(run_of)
    he[ids_sorted.long()] = run_of                      # (a permutation of [0, 3F): every entry is written)
    return he


def union_find(n, valid, pairs):
    """(labels [n] int32, number of components) of the graph on n nodes: hook + flatten, dense ids in the order of the components'
    minimum node index (syncs once: the number of components)."""
    dev = pairs.device
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n + 1, dtype=torch.int32, device=dev)
    call('nksr_uf_components', ptr(parent), n, ptr(valid), ptr(pairs), pairs.shape[0], ptr(flags), stream())
    rank = ops.exclusive_sum_i32(flags)
    ncomp = int(rank[n].item())
    label = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_uf_labels', ptr(parent), n, ptr(rank), ptr(label), stream())
    return label, ncomp


class Components:
    """Connected components of one mesh under one connectivity.  n; face_label [F] / vertex_label [V] int32 (-1: an invalid face, an
    unreferenced vertex); per component [n]: face_count, vertex_count, edge_count, boundary_edges, euler (int64), closed (bool), area
    (float64), box [n, 6] float32 (min xyz, max xyz).  Under 'edge' a vertex where components only touch carries the smallest of their
    ids and counts as a vertex of each."""

    def select(self, min_faces=0, min_area=0.0, min_area_ratio=0.0, keep_largest=None):
        """[n] bool: components with at least ``min_faces`` faces, an area of at least ``min_area`` and of at least ``min_area_ratio``
        times the LARGEST component's area; with ``keep_largest=k`` only the k largest of those by (area, then lower id)."""
        if min_faces < 0 or min_area < 0 or not 0.0 <= min_area_ratio <= 1.0:
            raise ValueError('select: min_faces, min_area must be >= 0 and min_area_ratio in [0, 1]')
        if keep_largest is not None and (isinstance(keep_largest, bool) or not isinstance(keep_largest, (int, np.integer)) or keep_largest < 0):
            raise ValueError('select: keep_largest must be a non-negative integer or None, got %r' % (keep_largest,))
        keep = (self.face_count >= int(min_faces)) & (self.area >= float(min_area))
        if self.n and min_area_ratio > 0.0:
            keep &= self.area >= float(min_area_ratio) * self.area.max()
        if keep_largest is not None and self.n:
            area = torch.where(keep, self.area, torch.full_like(self.area, -1.0))
            order = torch.sort(area, descending=True, stable=True)[1][:int(keep_largest)]       # (stable: the lower id first on a tie)
            top = torch.zeros_like(keep)
            top[order] = True
            keep &= top
        return keep

    def face_mask(self, keep):
        """[F] bool: faces of the components flagged in ``keep`` [n] (an invalid face: False)."""
        keep = torch.as_tensor(keep, device=self.face_label.device).to(torch.bool)
        if keep.shape != (self.n,):
            raise ValueError('face_mask: expected %d flags, got shape %s' % (self.n, tuple(keep.shape)))
        if self.n == 0:
            return torch.zeros(self.face_label.shape[0], dtype=torch.bool, device=self.face_label.device)
        return keep[self.face_label.clamp(min=0).long()] & (self.face_label >= 0)


def compact_mesh(v, f, face_keep, colors=None):
    """(v2, f2, c2, vertex_map): the kept valid faces in their order, the vertices they name in theirs, indices rewritten (syncs)."""
    nf, nv, dev = f.shape[0], v.shape[0], f.device
    fflags = torch.empty(nf + 1, dtype=torch.int32, device=dev)
    vflags = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    call('nksr_topo_compact_mark', ptr(f), is64(f), nf, nv, ptr(face_keep), ptr(fflags), ptr(vflags), stream())
    foffs, voffs = ops.exclusive_sum_i32(fflags), ops.exclusive_sum_i32(vflags)
    f2 = torch.empty((int(foffs[nf].item()), 3), dtype=f.dtype, device=dev)
    vmap = torch.empty(nv, dtype=torch.int64, device=dev)
    call('nksr_topo_compact_faces', ptr(f), is64(f), nf, nv, ptr(fflags), ptr(foffs), ptr(vflags), ptr(voffs), ptr(f2), ptr(vmap), stream())
    vkeep = vflags[:nv].bool()
    return v[vkeep], f2, None if colors is None else colors[vkeep], vmap


class MeshTopology:
    """Topology of one triangle mesh (v [V, 3], f [F, 3] int32 / int64) on the GPU; see the module's docstring."""

    def __init__(self, v, f, device=None):
        dev = gpu_device(device, like=v)
        vv = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
        rows3(vv, 'vertices')
        if not vv.dtype.is_floating_point:
            vv = vv.to(torch.float32)
        ff = mesh_input.faces(f, vv.shape[0], dev, cast_float=False, check_range=False)
        if vv.shape[0] >= 1 << 31:
            raise ValueError('mesh topology: %d vertices, at most 2^31 - 1' % vv.shape[0])
        if ff.shape[0] > TOPO_MAX_FACES:
            raise ValueError('mesh topology: %d faces, at most 2^30' % ff.shape[0])
        self._init(vv.to(dev).contiguous(), ff)

    @classmethod
    def from_device(cls, v, f, built=None):
        """A topology of tensors that are on the GPU already (v [V, 3] floating point, f [F, 3] int32 / int64, both contiguous)."""
        t = cls.__new__(cls)
        t._init(v, f, built)
        return t

    def _init(self, v, f, built=None):
        """Runs the stages; ``built`` = (face_valid, vertex_ref, keys_sorted, ids_sorted, EdgeTable) when the caller ran them itself."""
        self.device = v.device
        self.v = v                                              # the caller's precision: what compact() hands back
        self.v32 = v.to(torch.float32).contiguous()             # areas and boxes
        self.f = f
        self.n_vertices, self.n_faces = int(v.shape[0]), int(f.shape[0])
        if built is None:
            keys, ids, valid, ref = halfedge_keys(f, self.n_vertices)
            ks, ids_sorted = sort_halfedges(keys, ids, self.n_vertices)
            built = valid, ref, ks, ids_sorted, edge_runs(f, self.n_vertices, ks, ids_sorted, ref)
        self.face_valid, self.vertex_ref, self._keys_sorted, self._ids_sorted, self._table = built
        (self.num_edges, self.boundary_edges, self.nonmanifold_edges, self.misoriented_edges, self.invalid_faces,
         self.referenced_vertices) = self._table.totals
        self.edges, self.edge_counts = self._table.edges, self._table.edge_counts
        self.edge_classes, self.face_adjacency = self._table.edge_classes, self._table.face_adjacency
        self._components = {}
        self._halfedge_edge = None

    @property
    def halfedge_edge(self):
        """[3F] int32: the unique edge of half-edge 3 f + k, -1 for an invalid face (``halfedge_edges``; computed on first use and
        kept: the slicer and the boundary loops share it)."""
        if self._halfedge_edge is None:
            self._halfedge_edge = halfedge_edges(self._keys_sorted, self._ids_sorted, self.n_vertices)
        return self._halfedge_edge

    @property
    def euler_characteristic(self):
        return self.referenced_vertices - self.num_edges + (self.n_faces - self.invalid_faces)

    @property
    def is_closed(self):
        return self.boundary_edges == 0

    @property
    def is_edge_manifold(self):
        return self.nonmanifold_edges == 0

    @property
    def is_oriented(self):
        return self.misoriented_edges == 0

    @property
    def is_watertight(self):
        """Closed, edge-manifold and consistently oriented: then ``MeshQuery.occupancy`` is exact."""
        return self.is_closed and self.is_edge_manifold and self.is_oriented

    def components(self, connectivity='edge'):
        """``Components`` under 'edge' (faces joined across edges, non-manifold ones too) or 'vertex' (vertices joined by edges)."""
        if connectivity not in CONNECTIVITIES:
            raise ValueError("connectivity must be 'edge' or 'vertex', got %r" % (connectivity,))
        if connectivity not in self._components:
            self._components[connectivity] = self.component_stats(self.labels(connectivity))
        return self._components[connectivity]

    def labels(self, connectivity):
        """A ``Components`` with n and the labels only: hook + flatten, then the labels of the other kind of node."""
        nf, nv, dev = self.n_faces, self.n_vertices, self.device
        c = Components()
        if connectivity == 'edge':
            pairs = torch.empty((3 * nf, 2), dtype=torch.int32, device=dev)
            call('nksr_topo_face_pairs', ptr(self._keys_sorted), ptr(self._ids_sorted), 3 * nf, nv, ptr(pairs), stream())
            c.face_label, c.n = union_find(nf, self.face_valid, pairs)
            c.vertex_label = torch.empty(nv, dtype=torch.int32, device=dev)
        else:
            c.vertex_label, c.n = union_find(nv, self.vertex_ref, self.edges)
            c.face_label = torch.empty(nf, dtype=torch.int32, device=dev)
        call('nksr_topo_cross_labels', ptr(self.f), is64(self.f), nf, nv, ptr(self.face_valid), int(connectivity == 'vertex'),
             ptr(c.face_label), ptr(c.vertex_label), stream())
        c.connectivity = connectivity
        return c

    def component_stats(self, c):
        """Fills the per-component arrays of ``c`` (``labels``' result): integer counts by atomics, boxes by ordered-integer min / max,
        areas by a stable sort of the faces by label and a by-key scan."""
        v32, f, table, ids_sorted, connectivity = self.v32, self.f, self._table, self._ids_sorted, c.connectivity
        nf, nv, dev, n = f.shape[0], v32.shape[0], f.device, c.n
        ne = table.edges.shape[0]
        counts = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        c.box = torch.empty((n, 6), dtype=torch.float32, device=dev)
        c.area = torch.zeros(n, dtype=torch.float64, device=dev)
        if n:
            call('nksr_topo_component_counts', ptr(c.face_label), nf, ptr(c.vertex_label), nv, ptr(ids_sorted), ptr(table.edge_start),
                 ptr(table.edge_classes), ne, n, ptr(counts), stream())
            if connectivity == 'edge':          # vertices where components only touch: count them in every component (syncs: their number)
                m_dev = torch.empty(1, dtype=torch.int64, device=dev)
                call('nksr_topo_shared_corners', ptr(f), is64(f), nf, nv, ptr(c.face_label), ptr(c.vertex_label), None, 0, ptr(m_dev), stream())
                m = int(m_dev.item())
                if m:
                    keys = torch.empty(m, dtype=torch.int64, device=dev)
                    call('nksr_topo_shared_corners', ptr(f), is64(f), nf, nv, ptr(c.face_label), ptr(c.vertex_label), ptr(keys), m, ptr(m_dev), stream())
                    keys = ops.sort_keys(keys, end_bit=32 + int(n).bit_length())
                    call('nksr_topo_count_shared', ptr(keys), m, n, ptr(counts), stream())
            call('nksr_topo_component_boxes', ptr(v32), nv, ptr(f), is64(f), nf, ptr(c.face_label), n, ptr(c.box), stream())
            normal = torch.empty((nf, 3), dtype=torch.float32, device=dev)
            area = torch.empty(nf, dtype=torch.float64, device=dev)
            call('nksr_mesh_face_areas', ptr(v32), nv, ptr(f), is64(f), nf, ptr(normal), ptr(area), stream())
            key = torch.where(c.face_label >= 0, c.face_label, torch.full_like(c.face_label, n)).to(torch.int64)
            ks, order = ops.sort_pairs(key, torch.arange(nf, dtype=torch.int32, device=dev), end_bit=int(n).bit_length() + 1)
            sums = torch.empty(nf, dtype=torch.float64, device=dev)
            with_tmp('nksr_inclusive_sum_by_key_f64', dev, ptr(ks), ptr(area[order.long()].contiguous()), ptr(sums), nf, stream())
            c.area = sums[torch.cumsum(counts[:, 0], 0) - 1]            # (every component has a face: the last element of its segment)
        c.face_count, c.vertex_count, c.edge_count, c.boundary_edges = (counts[:, k].contiguous() for k in range(4))
        c.euler = c.vertex_count - c.edge_count + c.face_count
        c.closed = c.boundary_edges == 0
        return c

    def compact(self, face_keep, colors=None):
        """(v2, f2, c2, vertex_map [V] int64: new index or -1) of the faces flagged in ``face_keep`` [F] (invalid faces are dropped):
        faces and vertices keep their relative order, ``f2`` the dtype of the input, ``v2`` / ``c2`` rows of ``v`` / ``colors``."""
        keep = torch.as_tensor(face_keep).to(self.device)
        if keep.shape != (self.n_faces,):
            raise ValueError('compact: expected %d face flags, got shape %s' % (self.n_faces, tuple(keep.shape)))
        keep = (keep != 0).to(torch.uint8).contiguous()
        if colors is not None:
            colors = torch.as_tensor(colors).to(self.device)
            if colors.shape[0] != self.n_vertices:
                raise ValueError('compact: %d colour rows for %d vertices' % (colors.shape[0], self.n_vertices))
        return compact_mesh(self.v, self.f, keep, colors)

    def remove_small_components(self, min_faces=0, min_area=0.0, min_area_ratio=0.0, keep_largest=None, connectivity='edge', colors=None):
        """``compact`` of the components ``select`` keeps."""
        c = self.components(connectivity)
        return self.compact(c.face_mask(c.select(min_faces, min_area, min_area_ratio, keep_largest)), colors)
