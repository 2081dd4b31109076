"""Triangle-mesh clipping and tiling on the GPU: ``MeshClipper`` (plane splits, half-space and box clips, tile sets).

    c = MeshClipper(v, f, attr=None)            # v numpy / torch fp32 / fp64 on any device, f int32 / int64, attr [V, C] floating (the colours)
    c = MeshClipper.from_topology(t, attr=None) # reuse a MeshTopology: its edge table is the only set-up
    r = c.split(normal, offsets)                # ``SplitMesh``: ONE conforming mesh, every face cut along the planes n . x = offsets[j]
    p = r.parts()                               # ``Parts``: the exploded mesh, p[s] the MeshingResult between planes s - 1 and s
    m = c.clip(normal, offset, keep='above')    # MeshingResult of one side        m = c.clip_box(lo, hi)      # [lo, hi) per axis
    t = c.tiles(tile_size, origin=(0., 0.), axes=(0, 1))        # ``Tiles``: Parts on a grid, neighbours share bit-identical border vertices

Definition (kernels in csrc/meshclip.hip; restated in numpy by tests/mesh_clip_ref.py):
  heights     exactly ``nksr_slice_heights`` (mesh_slice.py).  The slab of a vertex is s_v = #{ j : o_j <= h_v } in [0, P]: the slicer's
              rule, a vertex exactly on a plane is above it.  Part s is { o_(s-1) <= h < o_s }; there are P + 1 parts.
  cut points  exactly the slicer's, from ``nksr_slice_counts`` and ``nksr_slice_points`` as they are: unique edge e carries the points of
              planes slab(min h) .. slab(max h) - 1, ids point_start[e] + (j - lo_e).  v2 = [the V input vertices ; the N points], point p
              has id V + p, and v2_64[V:] is bit-identical to ``MeshSlicer.slice(normal, offsets).points64``.
  pieces      a valid face (c0, c1, c2) is walked c0 -> c1 -> c2 -> c0.  On a half-edge a -> b the cut points come in travel order: planes
              s_a .. s_b - 1 ascending if s_a < s_b, planes s_a - 1 .. s_b descending if s_a > s_b.  A corner belongs to piece s_corner, a
              point of plane j to pieces j and j + 1.  Piece s (min s .. max s over the corners) is the cyclic subsequence of the walk's
              elements that belong to s: 3 to 5 vertices, convex, the face's orientation.
  triangles   every piece is fanned from its first element in the walk that starts at c0: (p0, p_i, p_i+1).  A face crossing k planes
              gives exactly 2 k + 1 triangles.  Output face id = face_start[f] + running index, face_start the exclusive scan of 2 k + 1
              over the faces (an invalid face counts 0); within a face the pieces ascend and a piece's triangles are in fan order.
              face_source[id] = f, face_part[id] = s.  Invalid faces are dropped (n_dropped).  Pieces that collapse because a vertex lies
              exactly on a plane are kept as zero-area triangles on coincident points, as the slicer keeps zero-length segments;
              n_degenerate counts the triangles with two corners of equal index or bit-identical position.
  attributes  attr2 = [attr ; a + t (b - a) per point] in fp64 from the canonical end points with the slicer's t, every operation rounded
              on its own.
  grouping    ``group_faces(f, labels, K)``: corner keys (label, vertex) sorted (``ops.sort_pairs``), one new vertex per run of the shared
              run table (``ops.sorted_runs``) -- numbered label-major, then by old vertex id -- and the faces stably sorted by label with
              their indices rewritten.  An original vertex lands in one part of a split, a cut point in the two parts it borders, so
              neighbouring parts and tiles carry bit-identical border vertices.
Every array repeats bit for bit: there is no atomic of any kind, ids are scans plus closed forms and every write has one writer.  ``split``
synchronises once (N, F2 and the piece count).  Limits: as MeshTopology, and V + N < 2^31, F2 < 2^31; ``parts`` needs 3 F2 < 2^31.
"""
import numpy as np
import torch

from . import mesh_slice as sl
from . import ops
from ._lib import call, ptr, stream
from .mesh_input import is64
from .mesh_slice import MeshSlicer
from .mesh_topology import MeshTopology, compact_mesh

LIMIT = 1 << 31
STAGES = ('heights', 'counts', 'points', 'faces', 'attr', 'group')      # 'counts' ends with the size read
FACES_BY_PIECE = 0          # nksr_clip_faces: one lane per face, the faster shape at every size measured (profiles/mesh_clip.md); 1: one lane per (face, piece)


def _result(v, f, c=None):
    from .fields.base_field import MeshingResult
    return MeshingResult(v, f, c)


# ---- stages (nksr_amd/tools/prof_mesh_clip.py times them one by one) ----------------------------------------------------------------
def face_starts(face_valid, seg_start):
    """(face_start, piece_start) [F + 1] int64: the exclusive scans of 2 k + 1 and of k + 1 over the valid faces, from the scan of k
    (``seg_start`` of ``mesh_slice.plane_ranges``) and the scan of the validity flags."""
    valid = torch.cat([face_valid.to(torch.int64), face_valid.new_zeros(1, dtype=torch.int64)])
    piece_start = seg_start + ops.exclusive_sum_i64(valid)
    return seg_start + piece_start, piece_start


def clip_faces(h, f, face_valid, he_edge, point_start, n_points, offsets, face_start, piece_start, n_pieces, n_out, by_piece=FACES_BY_PIECE):
    """(f2 [F2, 3], face_source [F2], face_part [F2]) int32."""
    dev = f.device
    f2 = torch.empty((n_out, 3), dtype=torch.int32, device=dev)
    source = torch.empty(n_out, dtype=torch.int32, device=dev)
    part = torch.empty(n_out, dtype=torch.int32, device=dev)
    call('nksr_clip_faces', ptr(h), h.shape[0], ptr(f), is64(f), f.shape[0], ptr(face_valid), ptr(he_edge), ptr(point_start), n_points, ptr(offsets),
         offsets.shape[0], ptr(face_start), ptr(piece_start), n_pieces, n_out, int(by_piece), ptr(f2), ptr(source), ptr(part), stream())
    return f2, source, part


def point_attr(attr, h, edges, offsets, point_edge, point_plane):
    """[N, C] fp64: ``attr`` [V, C] (fp32 / fp64) interpolated at the points."""
    n, ch = point_edge.shape[0], attr.shape[1]
    out = torch.empty((n, ch), dtype=torch.float64, device=attr.device)
    call('nksr_clip_attr', ptr(attr), int(attr.dtype == torch.float64), attr.shape[0], ch, ptr(h), ptr(edges), edges.shape[0], ptr(offsets),
         offsets.shape[0], ptr(point_edge), ptr(point_plane), n, ptr(out), stream())
    return out


def group_faces(f, labels, n_labels):
    """The exploded mesh of faces ``f`` [F, 3] int32 under ``labels`` [F] int32 in [0, K): (f_out [F, 3] int32 -- the faces stably sorted
    by label, indices into the new vertices --, face_order [F] int32 = the input face of every output face, vertex_source [R] int32 =
    the input vertex of every new vertex, part_vertex_start [K + 1], part_face_start [K + 1] int64).  Syncs once (R)."""
    nf, dev, k = f.shape[0], f.device, int(n_labels)
    if 3 * nf >= LIMIT:
        raise ValueError('mesh clipper: %d faces to group, 3 F at most 2^31 - 1' % nf)
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    ids = torch.empty(3 * nf, dtype=torch.int32, device=dev)
    call('nksr_clip_corner_keys', ptr(f), ptr(labels), nf, ptr(keys), ptr(ids), stream())
    ks, ids_sorted = ops.sort_pairs(keys, ids, end_bit=32 + max(k.bit_length(), 1))
    _, _, run_keys, run_of = ops.sorted_runs(ks, keys=True, run_of=True)
    corner_vertex = torch.empty_like(run_of)
    corner_vertex[ids_sorted.long()] = run_of               # (a permutation of [0, 3F): every entry is written)
    sorted_labels, order = ops.sort_pairs(labels.to(torch.int64), torch.arange(nf, dtype=torch.int32, device=dev), end_bit=max(k.bit_length(), 1))
    f_out = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    call('nksr_clip_group_faces', ptr(order), ptr(corner_vertex), nf, ptr(f_out), stream())
    bounds = torch.arange(k + 1, dtype=torch.int64, device=dev)
    return (f_out, order, (run_keys & 0xFFFFFFFF).to(torch.int32), torch.searchsorted(run_keys, bounds << 32),
            torch.searchsorted(sorted_labels, bounds))


class Parts:
    """A mesh exploded by face label: device tensors.  n_parts K; v64 [R, 3] fp64 and ``v`` in the caller's dtype, c [R, C] or None,
    f [F, 3] int32 (global indices into v, label order), labels [F] int32 (ascending), face_order [F] int32 (the face of the grouped
    mesh), vertex_source [R] int32 (its vertex), part_vertex_start / part_face_start [K + 1] int64.  ``parts[j]``: the MeshingResult
    (v, f, c) of part j with local indices, possibly empty; ``len`` = K; iteration yields the non-empty parts (``nonempty``: their ids)."""

    def __init__(self, v64, dtype, f, c, labels, n_labels):
        self.n_parts, self.dtype = int(n_labels), dtype
        self.f, self.face_order, self.vertex_source, self.part_vertex_start, self.part_face_start = group_faces(f, labels, n_labels)
        src = self.vertex_source.long()
        self.labels = labels[self.face_order.long()]
        self.v64 = v64[src]
        self.c = None if c is None else c[src]
        self._starts = None

    @property
    def v(self):
        return self.v64.to(self.dtype)

    def _host(self):
        if self._starts is None:
            self._starts = torch.stack([self.part_vertex_start, self.part_face_start]).tolist()        # (one host read for all parts)
        return self._starts

    def __len__(self):
        return self.n_parts

    @property
    def nonempty(self):
        fs = self._host()[1]
        return [j for j in range(self.n_parts) if fs[j + 1] > fs[j]]

    def __getitem__(self, j):
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= int(j) < self.n_parts:
            raise IndexError('part %r of %d' % (j, self.n_parts))
        vs, fs = self._host()
        a, b, fa, fb = vs[j], vs[j + 1], fs[j], fs[j + 1]
        return _result(self.v64[a:b].to(self.dtype), self.f[fa:fb] - a, None if self.c is None else self.c[a:b])

    def __iter__(self):
        return (self[j] for j in self.nonempty)


class Tiles(Parts):
    """``Parts`` on a grid: tile ix * ny + iy lies between levels ix - 1, ix of ``levels[0]`` along axes[0] and iy - 1, iy of ``levels[1]``
    along axes[1].  tile_index [K, 2] int32 = (ix, iy); shape = (nx, ny); axes; levels (two fp64 numpy arrays)."""


class SplitMesh:
    """The result of ``MeshClipper.split``: device tensors, integers int32 unless noted.  n_vertices V, n_points N, n_faces F2,
    n_parts P + 1, n_dropped (invalid input faces).  normal (three floats, unit), offsets [P] fp64, vertex_height [V] fp64;
    v2_64 [V + N, 3] fp64 (``v2``: the caller's dtype), f2 [F2, 3], attr2_64 [V + N, C] fp64 or None (``attr2``: the dtype of attr),
    face_part / face_source [F2], face_start [F + 1] int64, point_edge / point_plane [N], point_start [E + 1] int64."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._degenerate = None

    @property
    def v2(self):
        return self.v2_64.to(self.dtype)

    @property
    def attr2(self):
        return None if self.attr2_64 is None else self.attr2_64.to(self.attr_dtype)

    @property
    def n_degenerate(self):
        """Triangles with two corners of equal index or bit-identical position (one pass and one host read, on first use)."""
        if self._degenerate is None:
            p = self.v2_64.view(torch.int64)[self.f2.long()]            # [F2, 3, 3] position bits
            same = (p[:, 0] == p[:, 1]).all(1) | (p[:, 1] == p[:, 2]).all(1) | (p[:, 2] == p[:, 0]).all(1)
            self._degenerate = int(same.sum().item())
        return self._degenerate

    def parts(self, labels=None, n_labels=None):
        """``Parts`` by ``labels`` [F2] (integers in [0, n_labels); n_labels defaults to their maximum + 1), by default by ``face_part``."""
        if labels is None:
            labels, n_labels = self.face_part, self.n_parts
        else:
            labels = torch.as_tensor(labels)
            if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.shape != (self.n_faces,):
                raise ValueError('labels: expected %d integers, got %s %s' % (self.n_faces, labels.dtype, tuple(labels.shape)))
            labels = labels.to(self.f2.device)
            lo, hi = (int(labels.min()), int(labels.max())) if self.n_faces else (0, -1)
            n_labels = hi + 1 if n_labels is None else int(n_labels)
            if lo < 0 or hi >= n_labels or n_labels >= LIMIT:
                raise ValueError('labels: values in [%d, %d], expected [0, %d)' % (lo, hi, n_labels))
            labels = labels.to(torch.int32).contiguous()
        return Parts(self.v2_64, self.dtype, self.f2, self.attr2, labels, n_labels)

    def part(self, s):
        """The MeshingResult of part s alone, unused vertices dropped (``mesh_topology.compact_mesh``: the nksr_topo_compact_* path)."""
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < self.n_parts:
            raise IndexError('part %r of %d' % (s, self.n_parts))
        v, f, c, _ = compact_mesh(self.v2, self.f2, (self.face_part == int(s)).to(torch.uint8), self.attr2)
        return _result(v, f, c)


class MeshClipper:
    """Clipping of one triangle mesh (v [V, 3], f [F, 3] int32 / int64, attr [V, C]) on the GPU; see the module's docstring."""

    def __init__(self, v, f, attr=None, device=None):
        self._init(MeshTopology(v, f, device), attr)

    @classmethod
    def from_topology(cls, topology, attr=None):
        """The clipper over the edge table of a ``MeshTopology`` that exists already."""
        c = cls.__new__(cls)
        c._init(topology, attr)
        return c

    def _init(self, t, attr):
        self.slicer = MeshSlicer.from_topology(t)               # (refuses what is no MeshTopology)
        self.topology, self.device = t, t.device
        self.n_vertices, self.n_faces = t.n_vertices, t.n_faces
        self.attr = None
        if attr is not None:
            a = attr.detach() if isinstance(attr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(attr)))
            if not a.dtype.is_floating_point:
                raise ValueError('attr: expected floating-point values, got %s' % a.dtype)
            if a.dim() != 2 or a.shape[0] != t.n_vertices:
                raise ValueError('attr: shape %s for %d vertices' % (tuple(a.shape), t.n_vertices))
            self.attr = a.to(self.device).contiguous()

    def split(self, normal, offsets, _mark=None, _by_piece=None):
        """``SplitMesh`` along the planes { x : n . x = offsets[j] }, n = normal / |normal|; the arguments are ``MeshSlicer.slice``'s
        (ValueError otherwise), the offsets possibly empty: then the output is the valid faces unchanged.  A watertight input stays
        watertight.  (``_mark(stage)`` is called after every stage: the profiler's hook; ``_by_piece`` overrides FACES_BY_PIECE.)"""
        mark = _mark or (lambda stage: None)
        s, t, dev = self.slicer, self.topology, self.device
        n3 = MeshSlicer._unit(normal)
        off = s._offsets(offsets)
        nv, nf = self.n_vertices, self.n_faces
        h = sl.heights(s.x, n3)
        mark('heights')
        _, seg_start, lo_e, point_start = sl.plane_ranges(h, s.f, t.face_valid, t.edges, off)
        face_start, piece_start = face_starts(t.face_valid, seg_start)
        npts, nout, npieces, nseg = (int(c) for c in torch.stack([point_start[-1], face_start[-1], piece_start[-1], seg_start[-1]]).tolist())
        if nv + npts >= LIMIT or nout >= LIMIT:
            raise ValueError('mesh clipper: %d vertices + %d points and %d faces, at most 2^31 - 1 each' % (nv, npts, nout))
        mark('counts')
        points, point_edge, point_plane = sl.edge_points(s.x, h, t.edges, off, lo_e, point_start, npts)
        mark('points')
        f2, source, part = clip_faces(h, s.f, t.face_valid, s.halfedge_edge, point_start, npts, off, face_start, piece_start, npieces, nout,
                                      FACES_BY_PIECE if _by_piece is None else _by_piece)
        mark('faces')
        attr2 = None
        if self.attr is not None:
            a = self.attr if self.attr.dtype in (torch.float32, torch.float64) else self.attr.to(torch.float32)
            attr2 = torch.cat([a.to(torch.float64), point_attr(a, h, t.edges, off, point_edge, point_plane)])
        mark('attr')
        return SplitMesh(normal=n3, offsets=off, dtype=s.v.dtype, attr_dtype=None if self.attr is None else self.attr.dtype,
                         n_vertices=nv, n_points=npts, n_faces=nout, n_parts=int(off.shape[0]) + 1, n_dropped=nf - (npieces - nseg),
                         vertex_height=h, v2_64=torch.cat([s.x.to(torch.float64), points]), f2=f2, attr2_64=attr2, face_part=part,
                         face_source=source, face_start=face_start, point_edge=point_edge, point_plane=point_plane, point_start=point_start)

    def clip(self, normal, offset, keep='above'):
        """The MeshingResult (v, f, c = attr) of the side of the plane n . x = offset that ``keep`` names: 'above' is { n . x >= offset },
        'below' { n . x < offset }; cut faces are split along the plane and unused vertices dropped.  The section is left open: there is
        no cap (``MeshingResult.fill_holes`` closes simple sections)."""
        if keep not in ('above', 'below'):
            raise ValueError("keep must be 'above' or 'below', got %r" % (keep,))
        try:
            offset = float(offset)
        except (TypeError, ValueError):
            raise ValueError('offset: expected a number, got %r' % (offset,))
        return self.split(normal, [offset]).part(1 if keep == 'above' else 0)

    def clip_box(self, lo, hi):
        """The MeshingResult inside the box [lo, hi) per axis (the above-rule): three splits of two planes each, x then y then z, each
        keeping the middle part and run on the mesh the one before returned."""
        try:
            lo, hi = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (lo, hi))
        except (TypeError, ValueError):
            raise ValueError('clip_box: expected two corners of three numbers')
        if lo.shape != (3,) or hi.shape != (3,) or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
            raise ValueError('clip_box: expected finite corners with lo < hi on every axis, got %r, %r' % (lo.tolist(), hi.tolist()))
        c, m = self, None
        for axis in range(3):
            normal = [0.0, 0.0, 0.0]
            normal[axis] = 1.0
            m = c.split(normal, [lo[axis], hi[axis]]).part(1)
            if axis < 2:
                c = MeshClipper(m.v, m.f, m.c)
        return m

    def tiles(self, tile_size, origin=(0.0, 0.0), axes=(0, 1)):
        """``Tiles``: the mesh cut along the levels origin[i] + k tile_size of axes[i] in (min, max] over the referenced vertices
        (``MeshSlicer.interval_levels``, as ``contours(interval=)``): split along axes[0], that result split along axes[1], the faces
        labelled ix * ny + iy and grouped once."""
        try:
            axes, origin = tuple(axes), tuple(float(x) for x in origin)
        except (TypeError, ValueError):
            raise ValueError('tiles: expected two axes and a two-number origin')
        if len(axes) != 2 or len(origin) != 2 or any(isinstance(a, bool) or a not in (0, 1, 2) for a in axes) or axes[0] == axes[1]:
            raise ValueError('tiles: expected two different axes of 0, 1, 2 and a two-number origin, got %r, %r' % (axes, origin))
        levels = [self.slicer.interval_levels(tile_size, axes[i], origin[i]) for i in range(2)]
        nx, ny = len(levels[0]) + 1, len(levels[1]) + 1
        if nx * ny >= LIMIT:
            raise ValueError('tiles: %d x %d tiles, at most 2^31 - 1' % (nx, ny))
        normals = [[float(k == a) for k in range(3)] for a in axes]
        first = self.split(normals[0], levels[0])
        second = MeshClipper(first.v2, first.f2, first.attr2).split(normals[1], levels[1])
        labels = first.face_part[second.face_source.long()] * ny + second.face_part
        tiles = Tiles(second.v2_64, second.dtype, second.f2, second.attr2, labels.contiguous(), nx * ny)
        tiles.shape, tiles.axes, tiles.levels = (nx, ny), axes, levels
        k = torch.arange(nx * ny, dtype=torch.int32, device=self.device)
        tiles.tile_index = torch.stack([k // ny, k % ny], 1)
        tiles.first, tiles.second = first, second
        return tiles
