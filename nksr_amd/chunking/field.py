"""The blended field of a chunked scene: ``MultiChunkField`` (partition-of-unity blend of the parts, ownership of dual cells, the
mesh gather), its mask over UDF-masked chunks and the per-chunk views."""
import ctypes as C
import time
import weakref

import numpy as np
import torch

from .. import dist as D
from .._lib import call, ptr, stream
from ..fields.base_field import BaseField, EvaluationResult
from ..fields.mask_fields import LayerField, NeuralField
from ..svh import SparseFeatureHierarchy
from .geometry import chunk_grid_struct, chunk_index, chunk_pairs
from .payload import ChunkPart
from .residency import borrowed


class _ChunkViews:
    """``multi.fields``: per-chunk KernelFields, built on demand from the batch (the batch is what evaluates).  Holds the parts, not
    the MultiChunkField: a reference back to it would be a cycle, and the field (GBs of device memory) would then live until
    the cyclic collector happens to run instead of until its last reference goes."""

    def __init__(self, parts, part_of, interpolators):
        self._parts, self._part_of, self._interp, self._cache = parts, part_of, interpolators, {}

    def _ids(self):
        return sorted(self._part_of)

    def __iter__(self):
        return iter(self._ids())

    def __len__(self):
        return len(self._part_of)

    def __contains__(self, c):
        return c in self._part_of

    def keys(self):
        return self._ids()

    def __getitem__(self, c):
        if c not in self._cache:
            self._cache[c] = self._parts[self._part_of[c]].chunk_view(c, self._interp)
        return self._cache[c]

    def values(self):
        return [self[c] for c in self._ids()]

    def items(self):
        return [(c, self[c]) for c in self._ids()]


class ChunkUnionMask(BaseField):
    """Mask of a chunked field whose chunks carry NeuralField (UDF) masks: a vertex survives when any
    chunk that contributes to the blend there keeps it."""

    def __init__(self, multi):
        super().__init__(multi.svh)
        self._multi = weakref.ref(multi)          # the field owns its mask, not the other way round (no reference cycle)

    def evaluate_mask(self, xyz_model):
        m = self._multi()
        if m is None:
            raise RuntimeError('the chunked field this mask belongs to has been released')
        xyz_model = xyz_model.contiguous()
        keep = torch.zeros(xyz_model.shape[0], dtype=torch.bool, device=xyz_model.device)
        if xyz_model.shape[0] == 0:
            return keep
        _, q, cid, _, xq = m._pairs(xyz_model)
        pl = m._part_lut[cid.long()] if len(m.parts) > 1 else None
        for pi, part in enumerate(m.parts):
            if part.field.mask_field is None or not isinstance(part.field.mask_field, NeuralField):
                continue
            s = torch.nonzero(pl == pi).reshape(-1) if pl is not None else None
            qq, xx = (q, xq) if s is None else (q[s], xq[s].contiguous())
            if qq.numel():
                with borrowed(part.field, m.home) as pf:
                    kq = pf.mask_field.evaluate_mask(xx)
                keep[qq[kq]] = True          # a query may appear once per chunk: "any chunk keeps it"
        return keep

    def to_(self, device):
        return self


class MultiChunkField(BaseField):
    """Partition-of-unity blend of the chunk fields.  With one rank it holds every chunk and is valid everywhere.
    With several ranks a rank holds its own chunks in full and only the HALO of its spatial neighbours
    (chunking.exchange_band): ``evaluate_f`` is then exact inside the rank's own cores (+ the one-voxel ring it
    meshes) and must not be used elsewhere -- ``extract_dual_mesh`` respects that and gathers the pieces."""

    def __init__(self, parts, cores, ov, origin, chunk_size, grid, owner, rank, world_size, frame, interpolators, device, distributed=False,
                 adaptive_depth=1, halo_inner=None):
        self.parts = [p for p in parts if p.ids]
        self.halo_inner = halo_inner          # (model units; None: the lattice mesher's 2.5 voxels -- chunking.halo_inner)
        self.cores = cores                # {chunk id: (lo[3], hi[3])} model units
        self.ov = float(ov)
        self.origin, self.chunk_size, self.grid = origin, float(chunk_size), grid
        self.owner, self.rank, self.world_size = owner, rank, world_size
        self.frame, self.interpolators, self.distributed = frame, interpolators, bool(distributed)
        self.part_of = {c: i for i, p in enumerate(self.parts) for c in p.ids}
        nchunk = grid[0] * grid[1] * grid[2]
        lut = torch.full((nchunk,), -1, dtype=torch.long)
        shifts = np.zeros((nchunk, 3), np.float32)
        cells = np.zeros((nchunk, 3), np.int32)
        for c, i in self.part_of.items():
            lut[c] = i
            shifts[c] = frame.shift(c)
            cells[c] = frame.shift_cells(c)
        self._part_lut = lut.to(device)
        self._shift = torch.from_numpy(shifts).to(device)
        self._chunk_flag = self._part_lut.to(torch.int32)
        self._cgrid, self._cgrid_keep = chunk_grid_struct(origin, grid, chunk_size, None, self.ov, device, shift=self._shift)
        # union of the chunks' voxels on the GLOBAL lattice (integer translation back; T_c is a whole number of voxels at every
        # level): the dual grid that is meshed -- the finest level and, below adaptive_depth, the coarser ones (LayerField(dec_svh,
        # adaptive_depth), models/nksr_net.py:132; 2 in the carla preset, configs/carla/train.yaml:6)
        nlev = max(1, min(int(adaptive_depth), frame.depth))
        keys = [[] for _ in range(nlev)]
        for p in self.parts:
            kr = torch.tensor([frame.key_range(c)[0] for c in p.ids], dtype=torch.int64, device=device)
            sc_all = torch.from_numpy(cells[p.ids]).to(device)
            for d in range(min(nlev, p.field.svh.depth)):
                g = p.field.svh.level(d)
                if g.num_voxels == 0:
                    continue
                gk, gi = g.keys.to(device), g.ijk.to(device)              # (a parked part: its finest keys visit the GPU for this)
                seg = torch.bucketize(gk, kr >> (3 * d), right=True) - 1
                ijk = (gi - (sc_all[seg] >> d)).contiguous()
                k = torch.empty(ijk.shape[0], dtype=torch.int64, device=device)
                call('nksr_encode_keys', ptr(ijk), ijk.shape[0], d, ptr(k), stream())
                keys[d].append(k)
        union = SparseFeatureHierarchy(frame.w0, nlev, device)
        union.build_from_keys([torch.cat(k) if k else None for k in keys])
        super().__init__(union)
        self.meshing_depth = nlev
        self.mask_field = LayerField(union, nlev)
        if any(isinstance(p.field.mask_field, NeuralField) for p in self.parts):
            self.mask_field = ChunkUnionMask(self)
        self.solve_info = {}
        self.fields = _ChunkViews(self.parts, self.part_of, interpolators)
        self.home = torch.device(device)           # where evaluation and meshing run, wherever the parts are parked

    def chunk_infos(self):
        """[{'chunk', 'M', 'iters', 'rel_residual'}] of the chunks solved here (one host read per part)."""
        out = []
        for p in self.parts:
            info = p.field.solve_info
            if not p.solved or not info:
                continue
            si = info.get('segment_info')
            si = si.tolist() if si is not None else [[info['iters'], info['rel_residual']]]
            rg = p.ranges()
            for i, c in enumerate(p.ids):
                out.append({'chunk': c, 'M': sum(h - l for l, h in rg[c]), 'iters': int(si[i][0]), 'rel_residual': float(si[i][1])})
        return out

    # ---- blend ------------------------------------------------------------------------------------
    def _pairs(self, xyz):
        """(offsets [n + 1] int32, query index, chunk, weight, translated position) of every (query, chunk) with a positive blend
        weight, the pairs of a query in ASCENDING chunk order -- the fixed summation order of the blend (csrc/chunks.hip).  A
        chunk's weight is supported on core +- ov, so only the chunks around a query's home chunk are candidates."""
        return chunk_pairs(self._cgrid, 1, xyz, self._chunk_flag, True)

    def _evaluate_f_model(self, xyz, grad, max_points=1 << 22):
        n = xyz.shape[0]
        xyz = xyz.contiguous()
        f_out = torch.zeros(n, dtype=torch.float32, device=xyz.device)
        g_out = torch.zeros((n, 3), dtype=torch.float32, device=xyz.device) if grad else None
        if n == 0:
            return EvaluationResult(f_out, g_out)
        offs, _, cid, w, xq = self._pairs(xyz)
        m = xq.shape[0]
        if m == 0:                                 # no chunk weighs at any query: f = 0
            return EvaluationResult(f_out, g_out)
        # (a part parked on chunk_tmp_device / by to_('cpu') is borrowed for its evaluation: out-of-core, one part resident at a time)
        if len(self.parts) == 1:                   # one evaluation call per part for ALL pairs
            with borrowed(self.parts[0].field, self.home) as pf:
                res = pf._evaluate_f_model(xq, grad, max_points)
            f, gr = res.value.contiguous(), (res.gradient.contiguous() if grad else None)
        else:
            f = torch.empty(m, dtype=torch.float32, device=xyz.device)
            gr = torch.empty((m, 3), dtype=torch.float32, device=xyz.device) if grad else None
            pl = self._part_lut[cid.long()]
            for pi, part in enumerate(self.parts):
                s = torch.nonzero(pl == pi).reshape(-1)
                if s.numel():
                    with borrowed(part.field, self.home) as pf:
                        res = pf._evaluate_f_model(xq[s].contiguous(), grad, max_points)
                    f[s] = res.value
                    if grad:
                        gr[s] = res.gradient
        # f = sum w f_c / max(sum w, 1e-20); the gradient of the weights is ignored (they are flat outside the seams)
        call('nksr_chunk_blend', n, ptr(offs), ptr(w), ptr(f), ptr(gr) if grad else None, ptr(f_out), ptr(g_out) if grad else None, stream())
        return EvaluationResult(f_out, g_out)

    # ---- ownership of dual cells ----------------------------------------------------------------
    def chunk_of(self, xyz):
        return chunk_index(xyz, self.origin, self.grid, self.chunk_size)[1]

    def _whole_scene(self, t):
        """With one rank every cell and point is this rank's: the all-true mask over the rows of ``t``; None with several ranks."""
        return torch.ones(t.shape[0], dtype=torch.bool, device=t.device) if self.world_size == 1 else None

    def _owners(self, device):
        """``owner`` as an int32 device array (made on first use: a single rank never asks)."""
        if getattr(self, '_owner_dev', None) is None:
            self._owner_dev = torch.tensor(self.owner, dtype=torch.int32, device=device)
        return self._owner_dev

    def base_cell_mask(self, ijk):
        m = self._whole_scene(ijk)
        return m if m is not None else self.owns_points((ijk.to(torch.float32) + 0.5) * self.svh.voxel_size)

    def base_cell_halo_mask(self, ijk):
        """Owned cells plus one ring of neighbours: the MISE hanging-vertex rule needs to know whether
        the cells across a rank seam were refined, so they are evaluated (but not meshed) here too."""
        w = self.svh.voxel_size
        m = self._whole_scene(ijk)
        return m if m is not None else self.near_owned((ijk.to(torch.float32) + 0.5) * w, w)

    def seam_flags(self, edge_vkey, edge_axis, cells_per_voxel):
        """uint8 per mesh vertex of this rank's piece: 1 when another rank may emit the vertex too -- one of the four lattice cells
        around its edge is not this rank's (csrc/chunks.hip k_edge_seam_flags: base_cell_mask's arithmetic).  Rank 0 then groups only
        those (dist.merge_meshes)."""
        n = int(edge_vkey.numel())
        flags = torch.empty(n, dtype=torch.uint8, device=edge_vkey.device)
        if n:
            call('nksr_edge_seam_flags', C.byref(self._cgrid), ptr(edge_vkey.contiguous()), ptr(edge_axis.to(torch.int8).contiguous()), n, int(cells_per_voxel),
                 float(np.float32(self.svh.voxel_size)), ptr(self._owners(edge_vkey.device)), int(self.rank), ptr(flags), stream())
        return flags

    def _owner_flags(self, xyz, reach):
        """csrc/chunks.hip k_points_owner_flags: one launch instead of the ~100 torch launches of _near_owned_torch (same arithmetic)."""
        xyz = xyz.to(torch.float32).contiguous()
        n = xyz.shape[0]
        flags = torch.empty(n, dtype=torch.uint8, device=xyz.device)
        if n:
            call('nksr_points_owner_flags', C.byref(self._cgrid), ptr(xyz), n, float(np.float32(reach)), ptr(self._owners(xyz.device)), int(self.rank), ptr(flags), stream())
        return flags.bool()

    def owns_points(self, xyz):
        """Points (model units) inside a core this rank owns."""
        return self.near_owned(xyz, 0.0)

    def near_owned(self, centers, reach):
        """Points whose box centre +- ``reach`` (along the split axes) touches a core this rank owns."""
        m = self._whole_scene(centers)
        if m is not None:
            return m
        if centers.is_cuda:
            return self._owner_flags(centers, reach)
        return self._near_owned_torch(centers, reach)

    def _near_owned_torch(self, centers, reach):
        """near_owned in torch operations (the specification of k_points_owner_flags; tests compare the two)."""
        dev = centers.device
        own = torch.tensor(self.owner, dtype=torch.long, device=dev)
        w = reach
        # chunk index of centre - w / centre / centre + w along every split axis; only points next to a chunk
        # boundary (lo != hi on some axis) can see a different owner than their own chunk's
        split = [a for a in range(3) if self.grid[a] > 1]
        idx = {}
        for k, off in ((0, -w), (1, 0.0), (2, w)):
            for a, ia in enumerate(chunk_index(centers, self.origin, self.grid, self.chunk_size, off)[0]):
                idx[(a, k)] = ia

        def lin(sel, ks):
            out = torch.zeros(1, dtype=torch.long, device=dev)
            for a in range(3):
                ia = idx[(a, ks[a])][sel] if a in split else 0
                out = out * self.grid[a] + ia
            return out

        every = slice(None)
        m = own[lin(every, (1, 1, 1))] == self.rank
        near = torch.zeros(centers.shape[0], dtype=torch.bool, device=dev)
        for a in split:
            near |= idx[(a, 0)] != idx[(a, 2)]
        sel = torch.nonzero(near).reshape(-1)
        if sel.numel():
            ms = m[sel]
            combos = [()]
            for a in range(3):
                combos = [c + (k,) for c in combos for k in ((0, 1, 2) if a in split else (1,))]
            for ks in combos:
                ms = ms | (own[lin(sel, ks)] == self.rank)
            m[sel] = ms
        return m

    def _gathered(self, res, gather):
        """The bracket of the mesh gather: nothing to do for a single process; else ``gather(res)`` (point-to-point to rank 0 + the
        merge there, putting the merged arrays into ``res``) between two synchronisations, timed into ``last_gather_s``, and the
        colours of the merged vertices."""
        if self.world_size == 1 and not self.distributed:
            return res
        on_gpu = res.v.is_cuda and torch.cuda.is_available()      # (the gather also runs under gloo with CPU tensors: tests/test_dist_cpu.py)
        if on_gpu:
            torch.cuda.current_stream().synchronize()
        t0 = time.perf_counter()
        gather(res)
        if on_gpu:
            torch.cuda.current_stream().synchronize()
        self.last_gather_s = time.perf_counter() - t0
        res.c = self.texture_field.evaluate_color(res.v) if self.texture_field is not None else None
        return res

    def finalize_mesh(self, res):
        """The lattice mesher's pieces: gathered on rank 0, the vertices on rank seams merged there (dist.merge_meshes)."""
        def gather(res):
            res.v, res.f = D.gather_meshes(res.v, res.f, res.edge_vkey, res.edge_axis, seam=getattr(res, 'seam_flag', None))
        return self._gathered(res, gather)

    def finalize_mesh_named(self, res):
        """The adaptive dual graph's pieces: vertices named by the ordered pair of primal cells they join -- (size, key) names, the
        same on every rank -- gathered on rank 0 and merged there (dist.merge_named)."""
        def gather(res):
            res.v, res.f, res.vertex_names5 = D.gather_named(res.v, res.f, res.vertex_names5)
        return self._gathered(res, gather)

    def for_rank(self, rank, world_size, fields):
        """Same scene seen from another (simulated) rank holding the per-chunk ``fields`` -- test helper."""
        parts = [ChunkPart(f, [c], self.frame, solved=bool(f.solve_info)) for c, f in sorted(fields.items())]
        return MultiChunkField(parts, self.cores, self.ov, self.origin, self.chunk_size, self.grid, self.owner, rank,
                               world_size, self.frame, self.interpolators, self.svh.device, adaptive_depth=self.meshing_depth,
                               halo_inner=self.halo_inner)

    def to_(self, device):
        """``to_('cpu')`` parks the parts and the union grid on the host (NKSR-USAGE.md:163: "Put everything onto CPU"); evaluation
        and ``extract_dual_mesh`` keep running on the GPU the field was made on, borrowing one part at a time (out-of-core meshing:
        peak HBM = one part + the union grid + the lattice, not the scene).  The chunk tables (a few KB) stay where they are."""
        for p in self.parts:
            p.field.to_(device)
        self.svh.to_(device)
        return self

    def evaluate_f(self, xyz, grad=False):
        return super().evaluate_f(xyz.to(self.home), grad)

    @torch.no_grad()
    def extract_dual_mesh(self, mise_iter=0, grid_upsample=1, max_points=-1):
        with borrowed(self.svh, self.home):
            return super().extract_dual_mesh(mise_iter=mise_iter, grid_upsample=grid_upsample, max_points=max_points)
