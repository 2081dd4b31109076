"""Triangle-mesh simplification on the GPU: ``MeshSimplifier`` (quadric vertex clustering on a uniform grid, after Lindstrom).

    s = MeshSimplifier(v, f, colors=None)           # v numpy / torch fp32 / fp64 on any device, f int32 / int64, colors [V, C] floating
    s.count_faces(cell_size)                        # the number of faces simplify(cell_size) keeps; no quadrics
    r = s.simplify(cell_size=0.1)                   # or target_faces=n: the smallest cell size of a bisection with count <= n
    r.v2, r.f2, r.c2, r.vertex_map                  # dtypes of v, f, colors; vertex_map [V] int64: the new index or -1
    r.n_clusters, r.invalid_faces, r.collapsed_faces, r.duplicate_faces, r.cell_size, r.cluster_id [V] int32

Definitions (kernels in csrc/meshsimp.hip; restated in numpy by tests/mesh_simplify_ref.py):
  faces        a face with an index outside [0, V) or two equal indices is invalid: counted and ignored (as MeshTopology).  A vertex
               is referenced when a valid face names it; non-finite coordinates of referenced vertices are a ValueError.
  grid         origin = the fp64 componentwise minimum over the referenced vertices, or the caller's (<= that minimum on every axis,
               else ValueError).  Cell of a vertex: i = floor((double(x) - origin) / cell_size), an fp64 subtraction followed by an
               fp64 division, never a product with a reciprocal.  Every i < 2^21, else ValueError.  Key i_x << 42 | i_y << 21 | i_z;
               cluster ids are the ranks of the distinct keys, K their number.
  placement    relative to centre = origin + (i + 0.5) cell_size, in fp64.  mean = the mean of the cluster's referenced vertices.  For
               every corner of a valid face (collapsing ones too, once per corner) whose vertex lies in the cluster, with the face's
               unit normal n, area a and d = -n . (p0 - centre): A += a n n^T, b += a d n; a face without area adds nothing.
               x = (A + mu tau I)^-1 (-b + mu tau mean), tau = trace A, mu = ``regularisation`` (3 x 3 Cholesky; the matrix is positive
               definite with condition number <= 1 + 1 / mu); x = mean when tau = 0.  x is clamped to the cell, the representative is
               centre + x.  placement='mean': centre + mean.  Both rules are continuous in their inputs.
  faces out    a valid face maps to its corners' clusters in corner order and is dropped (collapsed) when two are equal; with
               ``dedup`` only the lowest-index face of every set of three clusters stays, whatever its orientation.  The kept faces
               keep their order; clusters no kept face names are dropped; v2 is in ascending key order.
  colours      c2 = the cluster means of ``colors``: fp64 sums over the cluster's referenced vertices in ascending vertex index.
  target       lo = diag / 2^20, hi = 2 diag (diag: the fp64 bounding-box diagonal of the referenced vertices); count(lo) <= n: lo;
               else 24 steps mid = sqrt(lo hi), count(mid) > n ? lo = mid : hi = mid; the answer is hi.  (A mesh without extent has
               one cluster at every cell size: cell_size 1.)
Every result repeats bit for bit: no floating-point atomic, every sum in the fixed order of a stably sorted run, the 16 partial sums
of a cluster in a fixed xor butterfly.  A different vertex or face order gives the same clusters and faces, and representatives that
differ by rounding.  Limits: as MeshTopology (V < 2^31, F <= 2^30), K < 2^31.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import mesh_input, ops
from ._lib import SIMP_MAX_INDEX, SIMP_MEAN, SIMP_QUADRIC, TOPO_MAX_FACES, call, ptr, stream
from .mesh_geometry import corner_incidence
from .mesh_input import gpu_device, is64, rows3
from .mesh_topology import compact_mesh

PLACEMENTS = {'quadric': SIMP_QUADRIC, 'mean': SIMP_MEAN}
BISECTION_STEPS = 24


def _origin3(origin):
    return (C.c_double * 3)(*[float(o) for o in origin])


# ---- stages (nksr_amd/tools/prof_mesh_simplify.py times them one by one) -------------------------------------------------------------
def reference_flags(f, nv):
    """(face_valid [F + 1], vertex_ref [V + 1]) int32: ``nksr_topo_compact_mark`` with every face kept."""
    nf, dev = f.shape[0], f.device
    fflags = torch.empty(nf + 1, dtype=torch.int32, device=dev)
    vflags = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    call('nksr_topo_compact_mark', ptr(f), is64(f), nf, nv, ptr(torch.ones(nf, dtype=torch.uint8, device=dev)), ptr(fflags), ptr(vflags), stream())
    return fflags, vflags


def cell_keys(x, vertex_ref, origin, cell_size):
    """(keys [V] int64, vertex ids [V] int32, the number of referenced vertices whose index does not fit)."""
    nv, dev = x.shape[0], x.device
    keys = torch.empty(nv, dtype=torch.int64, device=dev)
    ids = torch.empty(nv, dtype=torch.int32, device=dev)
    misfits = torch.empty(1, dtype=torch.int64, device=dev)
    call('nksr_simp_cell_keys', ptr(x), int(x.dtype == torch.float64), nv, ptr(vertex_ref), _origin3(origin), float(cell_size), ptr(keys), ptr(ids),
         ptr(misfits), stream())
    return keys, ids, misfits


class Clusters:
    """n; cluster_of [V] int32 (-1: unreferenced); start [K + 1] (uint32 in int32) into vertex_ids [V] (sorted by key, a run ascending);
    key [K] int64."""


def clusters(keys, ids, end_bit):
    """Stable sort over ``end_bit`` bits, then the runs of every key but the all-ones one (``ops.sorted_runs``; syncs once: K)."""
    ks, ids_sorted = ops.sort_pairs(keys, ids, end_bit=end_bit)
    c = Clusters()
    c.n, c.start, c.key, run_of = ops.sorted_runs(ks, keys=True, run_of=True)
    c.cluster_of = torch.empty_like(run_of)
    c.cluster_of[ids_sorted.long()] = run_of          # (a permutation of [0, V): every entry is written, unreferenced vertices with -1)
    c.vertex_ids = ids_sorted
    return c


class FaceMap:
    """cluster_faces [F, 3] (dtype of f), valid / survives [F] uint8, key_ab / key_c [F] int64, ids [F] int32, counts [2] int64."""


def face_remap(f, nv, cluster_of):
    nf, dev = f.shape[0], f.device
    m = FaceMap()
    m.cluster_faces = torch.empty((nf, 3), dtype=f.dtype, device=dev)
    m.valid = torch.empty(nf, dtype=torch.uint8, device=dev)
    m.survives = torch.empty(nf, dtype=torch.uint8, device=dev)
    m.key_ab = torch.empty(nf, dtype=torch.int64, device=dev)
    m.key_c = torch.empty(nf, dtype=torch.int64, device=dev)
    m.ids = torch.empty(nf, dtype=torch.int32, device=dev)
    m.counts = torch.empty(2, dtype=torch.int64, device=dev)
    call('nksr_simp_face_remap', ptr(f), is64(f), nf, nv, ptr(cluster_of), ptr(m.cluster_faces), ptr(m.valid), ptr(m.survives), ptr(m.key_ab),
         ptr(m.key_c), ptr(m.ids), ptr(m.counts), stream())
    return m


def flag_duplicates(m, nk):
    """(keep [F] uint8, duplicates [1] int64): two stable radix sorts, by c and then by (a, b), and one comparison with the predecessor."""
    nf, dev = m.ids.shape[0], m.ids.device
    bits = max(int(nk).bit_length(), 1)
    _, order = ops.sort_pairs(m.key_c, m.ids, end_bit=bits)
    _, order = ops.sort_pairs(m.key_ab[order.long()].contiguous(), order, end_bit=32 + bits)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    call('nksr_simp_flag_duplicates', ptr(order), nf, ptr(m.key_ab), ptr(m.key_c), ptr(m.survives), ptr(keep), ptr(count), stream())
    return keep, count


def place(x, f, corners, c, origin, cell_size, regularisation, placement):
    """[K, 3] fp64 representatives; ``corners`` = (corner_start [K + 1], corner_ids [3F]) or None under SIMP_MEAN."""
    out = torch.empty((c.n, 3), dtype=torch.float64, device=x.device)
    start, ids = corners if corners is not None else (None, None)
    call('nksr_simp_place', ptr(x), int(x.dtype == torch.float64), x.shape[0], ptr(f), is64(f), f.shape[0], ptr(start), ptr(ids), ptr(c.start),
         ptr(c.vertex_ids), ptr(c.key), c.n, _origin3(origin), float(cell_size), float(regularisation), placement, ptr(out), stream())
    return out


def cluster_means(attr, c):
    """[K, C] fp64 means of attr [V, C] (fp32 / fp64) over the clusters' vertex runs."""
    out = torch.empty((c.n, attr.shape[1]), dtype=torch.float64, device=attr.device)
    call('nksr_simp_cluster_means', ptr(attr), int(attr.dtype == torch.float64), attr.shape[0], attr.shape[1], ptr(c.start), ptr(c.vertex_ids), c.n,
         ptr(out), stream())
    return out


class SimplifyResult:
    """v2 [V2, 3], f2 [F2, 3], c2 [V2, C] or None, vertex_map [V] int64, cluster_id [V] int32, n_clusters, invalid_faces, collapsed_faces,
    duplicate_faces, cell_size."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class MeshSimplifier:
    """Simplification of one triangle mesh (v [V, 3], f [F, 3] int32 / int64, colors [V, C]) on the GPU; see the module's docstring."""

    def __init__(self, v, f, colors=None, device=None):
        dev = gpu_device(device, like=v)
        vv = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
        rows3(vv, 'vertices')
        if not vv.dtype.is_floating_point:
            vv = vv.to(torch.float32)
        ff = mesh_input.faces(f, vv.shape[0], dev, cast_float=False, check_range=False)
        if vv.shape[0] >= 1 << 31:
            raise ValueError('mesh simplifier: %d vertices, at most 2^31 - 1' % vv.shape[0])
        if ff.shape[0] > TOPO_MAX_FACES:
            raise ValueError('mesh simplifier: %d faces, at most 2^30' % ff.shape[0])
        cc = None
        if colors is not None:
            cc = colors.detach() if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(colors)))
            if not cc.dtype.is_floating_point:
                raise ValueError('colors: expected floating-point values, got %s' % cc.dtype)
            if cc.dim() != 2 or cc.shape[0] != vv.shape[0]:
                raise ValueError('colors: shape %s for %d vertices' % (tuple(cc.shape), vv.shape[0]))
            cc = cc.to(dev).contiguous()
        self.device, self.v, self.f, self.colors = dev, vv.to(dev).contiguous(), ff, cc
        self.x = self.v if self.v.dtype in (torch.float32, torch.float64) else self.v.to(torch.float32)      # what the kernels read
        self.n_vertices, self.n_faces = int(vv.shape[0]), int(ff.shape[0])
        self.face_valid, self.vertex_ref = reference_flags(ff, self.n_vertices)
        ref = self.vertex_ref[:self.n_vertices].bool()
        pts = self.x[ref].to(torch.float64)
        self.referenced_vertices = int(pts.shape[0])
        self.invalid_faces = self.n_faces - int(self.face_valid.sum().item())
        self.box = None                     # fp64 (min [3], max [3]) over the referenced vertices
        if self.referenced_vertices:
            if not bool(torch.isfinite(pts).all()):
                raise ValueError('vertices: non-finite coordinates')
            self.box = pts.amin(0).tolist(), pts.amax(0).tolist()

    @property
    def diagonal(self):
        if self.box is None:
            return 0.0
        d = [hi - lo for lo, hi in zip(*self.box)]
        return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])

    # ---- arguments ----
    @staticmethod
    def _cell(cell_size):
        try:
            h = float(cell_size)
        except (TypeError, ValueError):
            raise ValueError('cell_size must be a positive finite number, got %r' % (cell_size,))
        if not (h > 0.0 and math.isfinite(h)):
            raise ValueError('cell_size must be a positive finite number, got %r' % (cell_size,))
        return h

    def _grid(self, h, origin):
        """(origin [3] floats, the sort's key bits); the ValueErrors of the grid."""
        if origin is not None:
            origin = [float(o) for o in np.asarray(origin, np.float64).reshape(-1)]
            if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
                raise ValueError('origin: expected three finite numbers, got %r' % (origin,))
        if self.box is None:
            return origin or [0.0, 0.0, 0.0], 1
        lo, hi = self.box
        if origin is None:
            origin = list(lo)
        elif any(o > m for o, m in zip(origin, lo)):
            raise ValueError('origin %r lies above the minimum %r of the referenced vertices' % (origin, lo))
        extent = [math.floor((m - o) / h) for m, o in zip(hi, origin)]      # (floor of an fp64 subtraction and division: the kernel's own index)
        if max(extent) >= SIMP_MAX_INDEX:
            raise ValueError('cell_size %r puts the grid extent at %r cells, at most 2^21 per axis' % (h, [e + 1 for e in extent]))
        bits = 42 + extent[0].bit_length() if extent[0] else (21 + extent[1].bit_length() if extent[1] else extent[2].bit_length())
        return origin, (64 if self.referenced_vertices < self.n_vertices else max(bits, 1))      # (the all-ones key differs in every bit)

    # ---- the passes ----
    def _faces(self, h, origin, dedup):
        """Clusters, the face map, the keep flags and the duplicate count; None without referenced vertices (syncs: K, misfits)."""
        origin, bits = self._grid(h, origin)
        if self.box is None:
            return None
        keys, ids, misfits = cell_keys(self.x, self.vertex_ref, origin, h)
        c = clusters(keys, ids, bits)
        if int(misfits.item()):
            raise ValueError('cell_size %r: %d vertices fall outside the 2^21 cells per axis' % (h, int(misfits.item())))
        m = face_remap(self.f, self.n_vertices, c.cluster_of)
        if dedup:
            keep, dups = flag_duplicates(m, c.n)
        else:
            keep, dups = m.survives, None
        return origin, c, m, keep, dups

    def count_faces(self, cell_size, origin=None, dedup=True):
        """The number of faces ``simplify(cell_size, origin=origin, dedup=dedup)`` keeps."""
        got = self._faces(self._cell(cell_size), origin, dedup)
        return 0 if got is None else int(got[3].sum().item())

    def target_cell_size(self, target_faces, origin=None, dedup=True):
        """The cell size of the bisection in the module's docstring: ``count_faces`` of it is <= target_faces."""
        diag = self.diagonal
        if diag == 0.0:
            return 1.0
        lo, hi = diag / 2.0 ** 20, 2.0 * diag
        if self.count_faces(lo, origin, dedup) <= target_faces:
            return lo
        for _ in range(BISECTION_STEPS):
            mid = math.sqrt(lo * hi)
            if self.count_faces(mid, origin, dedup) > target_faces:
                lo = mid
            else:
                hi = mid
        return hi

    def simplify(self, cell_size=None, target_faces=None, origin=None, placement='quadric', regularisation=1e-3, dedup=True):
        """A ``SimplifyResult``; exactly one of ``cell_size`` and ``target_faces``."""
        if (cell_size is None) == (target_faces is None):
            raise ValueError('give exactly one of cell_size and target_faces')
        if placement not in PLACEMENTS:
            raise ValueError("placement must be 'quadric' or 'mean', got %r" % (placement,))
        mu = float(regularisation)
        if not 0.0 < mu <= 1.0:
            raise ValueError('regularisation must lie in (0, 1], got %r' % (regularisation,))
        if target_faces is not None:
            if isinstance(target_faces, bool) or int(target_faces) != target_faces or target_faces < 0:
                raise ValueError('target_faces must be a non-negative integer, got %r' % (target_faces,))
            h = self.target_cell_size(int(target_faces), origin, dedup)
        else:
            h = self._cell(cell_size)
        nv, dev = self.n_vertices, self.device
        got = self._faces(h, origin, dedup)
        if got is None:                     # no valid face: nothing is referenced, nothing is kept
            c2 = None if self.colors is None else self.colors[:0].clone()
            return SimplifyResult(v2=self.v[:0].clone(), f2=self.f[:0].clone(), c2=c2, vertex_map=torch.full((nv,), -1, dtype=torch.int64, device=dev),
                                  cluster_id=torch.full((nv,), -1, dtype=torch.int32, device=dev), n_clusters=0, invalid_faces=self.invalid_faces,
                                  collapsed_faces=0, duplicate_faces=0, cell_size=h)
        origin, c, m, keep, dups = got
        corners = corner_incidence(m.cluster_faces, m.valid, c.n) if placement == 'quadric' else None
        rep = place(self.x, self.f, corners, c, origin, h, mu, PLACEMENTS[placement])
        means = None
        if self.colors is not None:
            col = self.colors if self.colors.dtype in (torch.float32, torch.float64) else self.colors.to(torch.float32)
            means = cluster_means(col, c)
        rep2, f2, c2, cmap = compact_mesh(rep, m.cluster_faces, keep, means)
        vertex_map = torch.where(c.cluster_of >= 0, cmap[c.cluster_of.clamp(min=0).long()], cmap.new_full((), -1))
        counts = m.counts.tolist()
        return SimplifyResult(v2=rep2.to(self.v.dtype), f2=f2, c2=None if c2 is None else c2.to(self.colors.dtype), vertex_map=vertex_map,
                              cluster_id=c.cluster_of, n_clusters=c.n, invalid_faces=int(counts[0]), collapsed_faces=int(counts[1]),
                              duplicate_faces=0 if dups is None else int(dups.item()), cell_size=h)
