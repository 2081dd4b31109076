"""Field base class -- host-side mirror of ``nksr.fields`` (base part).

Reference interface (call sites): ``field.extract_dual_mesh(mise_iter=, grid_upsample=,
max_points=)`` -> object with ``.v .f .c`` (examples/recons_simple.py:27,
recons_colored_mesh.py:30, models/nksr_net.py:214,284; NKSR-USAGE.md:52,79);
``field.evaluate_f(xyz, grad=)`` -> ``.value`` / ``.gradient`` (models/loss.py:189-198);
``set_mask_field`` / ``.mask_field`` / ``.svh`` (models/nksr_net.py:133, models/loss.py:132-133);
``set_texture_field`` (recons_colored_mesh.py:28); ``to_`` (NKSR-USAGE.md:163).
"""
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class EvaluationResult:
    value: torch.Tensor
    gradient: Optional[torch.Tensor] = None


@dataclass
class MeshingResult:
    v: torch.Tensor
    f: torch.Tensor
    c: Optional[torch.Tensor] = None

    def topology(self):
        """``MeshTopology`` of this mesh (nksr_amd/mesh_topology.py): edge classes, Euler characteristic, components."""
        from ..mesh_topology import MeshTopology
        return MeshTopology(self.v, self.f)

    def remove_small_components(self, min_faces=0, min_area=0.0, min_area_ratio=0.0, keep_largest=None, connectivity='edge'):
        """A new ``MeshingResult`` without the components below the thresholds (``Components.select``), ``c`` carried through."""
        v, f, c, _ = self.topology().remove_small_components(min_faces, min_area, min_area_ratio, keep_largest, connectivity, self.c)
        return MeshingResult(v, f, c)

    def geometry(self):
        """``MeshGeometry`` of this mesh (nksr_amd/mesh_geometry.py): adjacency, normals, curvature, smoothing."""
        from ..mesh_geometry import MeshGeometry
        return MeshGeometry(self.v, self.f)

    def vertex_normals(self, weighting='angle'):
        """[V, 3] unit vertex normals in the dtype of ``v`` (``MeshGeometry.vertex_normals``)."""
        return self.geometry().vertex_normals(weighting)

    def smooth(self, iterations, method='taubin', lam=0.5, mu=-0.53, boundary='fixed', fixed=None):
        """A new ``MeshingResult`` with the vertices of ``MeshGeometry.smooth``; ``f`` and ``c`` are shared with this one."""
        return MeshingResult(self.geometry().smooth(iterations, method, lam, mu, boundary, fixed), self.f, self.c)

    def simplify(self, cell_size=None, target_faces=None, **kw):
        """A new ``MeshingResult`` from ``MeshSimplifier.simplify`` (nksr_amd/mesh_simplify.py): the vertices of one grid cell become
        one, placed by the quadrics of its faces; ``c`` is averaged per cell.  ``kw``: origin, placement, regularisation, dedup."""
        from ..mesh_simplify import MeshSimplifier
        r = MeshSimplifier(self.v, self.f, self.c).simplify(cell_size=cell_size, target_faces=target_faces, **kw)
        return MeshingResult(r.v2, r.f2, r.c2)

    def slice(self, normal, offsets):
        """``Sections`` of this mesh on the planes n . x = offsets[j] (``MeshSlicer.slice``, nksr_amd/mesh_slice.py): points on the
        edges, one segment per face and plane, and the segments ordered into polylines with their lengths and signed areas."""
        from ..mesh_slice import MeshSlicer
        return MeshSlicer(self.v, self.f).slice(normal, offsets)

    def contours(self, levels=None, interval=None, axis=2):
        """``Sections`` at ``levels`` along ``axis``, or at the multiples of ``interval`` (``MeshSlicer.contours``)."""
        from ..mesh_slice import MeshSlicer
        return MeshSlicer(self.v, self.f).contours(levels=levels, interval=interval, axis=axis)

    def split(self, normal, offsets):
        """``SplitMesh`` of this mesh along the planes n . x = offsets[j] (``MeshClipper.split``, nksr_amd/mesh_clip.py): one conforming
        mesh whose faces are cut along the planes, ``c`` interpolated at the cut points; ``.parts()`` explodes it."""
        from ..mesh_clip import MeshClipper
        return MeshClipper(self.v, self.f, self.c).split(normal, offsets)

    def clip(self, normal, offset, keep='above'):
        """A new ``MeshingResult``: the side of the plane n . x = offset that ``keep`` names (``MeshClipper.clip``); no cap."""
        from ..mesh_clip import MeshClipper
        return MeshClipper(self.v, self.f, self.c).clip(normal, offset, keep)

    def clip_box(self, lo, hi):
        """A new ``MeshingResult``: what lies inside the box [lo, hi) (``MeshClipper.clip_box``)."""
        from ..mesh_clip import MeshClipper
        return MeshClipper(self.v, self.f, self.c).clip_box(lo, hi)

    def tiles(self, tile_size, origin=(0.0, 0.0), axes=(0, 1)):
        """``Tiles`` of this mesh on a grid of ``tile_size`` along ``axes`` (``MeshClipper.tiles``): neighbours meet without cracks."""
        from ..mesh_clip import MeshClipper
        return MeshClipper(self.v, self.f, self.c).tiles(tile_size, origin, axes)

    def height_map(self, pixel_size, origin=None, shape=None, axes=(0, 1), surface='top'):
        """``HeightMap`` of this mesh on a regular grid (``MeshRasterizer.height_map``, nksr_amd/mesh_raster.py): elevation, covering
        face and layer count per pixel on the lattice origin + k pixel_size that ``tiles`` and ``contours`` cut at; ``sample()`` on it
        resamples the colours ``c`` (an orthoimage), ``slope()`` and ``hillshade()`` derive from it."""
        from ..mesh_raster import MeshRasterizer
        return MeshRasterizer(self.v, self.f, self.c).height_map(pixel_size, origin, shape, axes, surface)

    def boundary_loops(self):
        """``BoundaryLoops`` of this mesh (``MeshBoundary.loops``, nksr_amd/mesh_boundary.py): the boundary edges ordered into loops
        with their edge counts, lengths, areas, centroids and boxes."""
        from ..mesh_boundary import MeshBoundary
        return MeshBoundary(self.v, self.f).loops()

    def fill_holes(self, max_edges=None, max_length=None, max_area=None, method='centroid'):
        """A new ``MeshingResult`` with the closed, simple boundary loops at or under the thresholds closed (``BoundaryLoops.select``,
        ``MeshBoundary.fill``), ``c`` carried through.  Without a threshold every closed loop is filled, the rim of an open surface
        included."""
        from ..mesh_boundary import MeshBoundary
        b = MeshBoundary(self.v, self.f)
        v, f, c, _, _ = b.fill(b.loops().select(max_edges, max_length, max_area), method, self.c)
        return MeshingResult(v, f, c)


class BaseField:
    def __init__(self, svh):
        self.svh = svh
        self.scale = 1.0          # world -> model units (Reconstructor's global scale)
        self.mask_field = None
        self.texture_field = None
        self.meshing_depth = 1     # levels whose dual cells are meshed (Reconstructor sets hparams.adaptive_depth)
        self.dual_graph = 'lattice'     # or 'adaptive': marching cubes on the dual graph of the flattened levels (meshing._extract_adaptive)

    @property
    def device(self):
        return self.svh.device

    def set_scale(self, scale):
        self.scale = float(scale)

    def set_mask_field(self, mask_field):
        self.mask_field = mask_field

    def set_texture_field(self, texture_field):
        self.texture_field = texture_field

    # model-unit evaluation, implemented by subclasses
    def _evaluate_f_model(self, xyz, grad):
        raise NotImplementedError

    def evaluate_f(self, xyz, grad=False):
        """f (and optionally its gradient) at world-space positions."""
        xyz = xyz.to(torch.float32)
        if self.scale != 1.0:
            xyz = xyz * self.scale
        res = self._evaluate_f_model(xyz.contiguous(), grad)
        if grad and res.gradient is not None and self.scale != 1.0:
            res.gradient = res.gradient * self.scale
        return res

    def evaluate_f_bar(self, xyz):
        """Value used for occupancy tests: f > 0 <=> inside (models/loss.py:99-100)."""
        return self.evaluate_f(xyz, grad=False).value

    def mask_vertices(self, xyz_model):
        """True where a mesh vertex (model units) survives trimming."""
        if self.mask_field is None:
            return None
        return self.mask_field.evaluate_mask(xyz_model)

    @torch.no_grad()       # a mesh is not differentiated: plain evaluation of the lattice values
    def extract_dual_mesh(self, mise_iter=0, grid_upsample=1, max_points=-1):
        from .. import meshing
        return meshing.extract_dual_mesh(self, mise_iter=mise_iter, grid_upsample=grid_upsample, max_points=max_points)

    def to_(self, device):
        raise NotImplementedError
