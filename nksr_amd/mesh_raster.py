"""Triangle-mesh rasterisation on the GPU: ``MeshRasterizer`` (height maps, orthoimages, slope and hillshade on a regular grid).

    r  = MeshRasterizer(v, f, attr=None)        # v numpy / torch fp32 / fp64 on any device, f int32 / int64, attr [V, C] floating (the colours)
    hm = r.height_map(pixel_size, origin=None, shape=None, axes=(0, 1), surface='top')          # ``HeightMap``
    hm.height, hm.face, hm.count, hm.valid      # [nx, ny]: fp64 (NaN where empty), int32 (-1 where empty), int32, bool
    hm.layers()                                 # every covering of every pixel, per pixel in ascending face id
    hm.sample(attr=None), hm.gradient(), hm.slope(), hm.hillshade(azimuth=315.0, altitude=45.0)

Definition (kernels in csrc/meshraster.hip; restated in numpy by tests/mesh_raster_ref.py):
  frame       x = v[:, axes[0]], y = v[:, axes[1]], z = v[:, up], up = 3 - axes[0] - axes[1]; read in the caller's precision and widened
              to fp64 exactly.  No recentring: every difference is taken in fp64.  surface 'top' keeps the largest z per pixel, 'bottom'
              the smallest.
  grid        pixel (i, j) has the centre X_i = origin[0] + (i + 0.5) p, Y_j = origin[1] + (j + 0.5) p: one rounded product and one
              rounded sum.  Rasters are [nx, ny], flat index i ny + j.  origin=None: floor(min / p) p over the referenced vertices of
              the valid faces; shape=None: floor((max - origin) / p) + 1 per axis.  The lattice origin + k p is the one ``tiles`` and
              ``contours(interval=)`` cut at.
  validity    a face with an index outside [0, V) or a corner that is not finite is dropped and counted (n_dropped).
  coverage    with A = (x_a - X_i, y_a - Y_j), B, C likewise and e(P, Q) = Px Qy - Py Qx (two rounded products, one subtraction):
              s(P, Q) = sign(e) if e != 0, else sign(Py - Qy) if Py != Qy, else sign(Qx - Px): antisymmetric bit for bit, so the two
              faces of an edge never both claim a centre on it and never both miss it, whatever their winding.  U = e(B, C),
              V = e(C, A), W = e(A, B); the face covers the centre iff s_U = s_V = s_W != 0 and det = (U + V) + W != 0.  A centre on
              the outer border of a region belongs to it on the low sides and not on the high ones: the [lo, hi) rule of ``clip_box``.
  height      zf = ((U z_a + V z_b) + W z_c) / det; an attribute likewise per channel.
  per pixel   count = the covering faces, height = the max (top) / min (bottom) of their zf, face = the lowest face id that attains it.
  gradient    Horn: gx = (((h[i+1,j-1] + 2 h[i+1,j]) + h[i+1,j+1]) - ((h[i-1,j-1] + 2 h[i-1,j]) + h[i-1,j+1])) / (8 p), gy the same
              along j; NaN on the rim and beside an empty pixel.
  hillshade   max(0, (s_z - (s_x gx + s_y gy)) / sqrt((1 + gx gx) + gy gy)), (s_x, s_y, s_z) the unit vector to the sun (``sun_vector``:
              numpy fp64 on the host; azimuth clockwise from +axes[1], altitude above the horizon, degrees).
Passes: a candidate box per face (one pixel of margin), one lane per (face, pixel of its box) for the predicate, a scan of the flags and
a compaction to hits, a stable sort of the hits by pixel, the shared run table, one lane per run for the rasters.  Every array repeats
bit for bit: there is no atomic of any kind and every write has one writer.  ``height_map`` synchronises for the extent of the mesh, for
the candidate count, for the hit count and in ``ops.sorted_runs``.  Limits: V < 2^31, F <= 2^30, nx ny < 2^31, candidates and hits
< 2^31 each (ValueError: use a larger pixel or rasterise ``tiles``).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import mesh_input, ops
from ._lib import RASTER_BLOCK, TOPO_MAX_FACES, call, ptr, stream
from .mesh_input import gpu_device, is64, rows3

LIMIT = 1 << 31
MIN_PIXEL_RATIO = 2.0 ** -40        # of the largest |x|, |y| or |origin|: below it the one-pixel margin of the boxes no longer covers the rounding
SURFACES = ('top', 'bottom')
STAGES = ('boxes', 'test', 'compact', 'sort', 'reduce')         # 'boxes', 'compact' and 'sort' end with a size read


# ---- arguments (no GPU needed) ------------------------------------------------------------------------------------------------------
def raster_axes(axes):
    """(axes[0], axes[1], up) of two different axes of 0, 1, 2 (the rules of ``MeshClipper.tiles``), else ValueError."""
    try:
        axes = tuple(axes)
    except TypeError:
        raise ValueError('axes: expected two different values of 0, 1, 2, got %r' % (axes,))
    if len(axes) != 2 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a not in (0, 1, 2) for a in axes) or axes[0] == axes[1]:
        raise ValueError('axes: expected two different values of 0, 1, 2, got %r' % (axes,))
    return int(axes[0]), int(axes[1]), 3 - int(axes[0]) - int(axes[1])


def raster_grid(pixel_size, origin, shape, extent):
    """(p, (ox, oy), (nx, ny)) of a height map over a mesh whose valid faces span ``extent`` = (xmin, xmax, ymin, ymax) along the two
    raster axes (None: no valid face), or ValueError.  Pure host arithmetic in fp64: it needs no GPU."""
    try:
        p = float(pixel_size)
    except (TypeError, ValueError):
        raise ValueError('pixel_size must be a positive finite number, got %r' % (pixel_size,))
    if not (p > 0.0 and math.isfinite(p)):
        raise ValueError('pixel_size must be a positive finite number, got %r' % (pixel_size,))
    if extent is not None:
        extent = tuple(float(e) for e in extent)
        if len(extent) != 4 or not all(math.isfinite(e) for e in extent):
            raise ValueError('extent: expected four finite numbers, got %r' % (extent,))
    if origin is None:
        origin = (0.0, 0.0) if extent is None else (math.floor(extent[0] / p) * p, math.floor(extent[2] / p) * p)
    else:
        try:
            origin = tuple(float(o) for o in origin)
        except (TypeError, ValueError):
            raise ValueError('origin: expected two numbers, got %r' % (origin,))
    if len(origin) != 2 or not all(math.isfinite(o) for o in origin):
        raise ValueError('origin: expected two finite numbers, got %r' % (origin,))
    largest = max([abs(o) for o in origin] + [abs(e) for e in extent or ()])
    if p < MIN_PIXEL_RATIO * largest:
        raise ValueError('pixel_size %r is below 2^-40 of the largest coordinate magnitude %r: the grid cannot be resolved in fp64' % (p, largest))
    if shape is None:
        shape = (0, 0) if extent is None else tuple(max(math.floor((extent[2 * k + 1] - origin[k]) / p) + 1, 0) for k in range(2))
    else:
        try:
            shape = tuple(shape)
        except TypeError:
            raise ValueError('shape: expected two non-negative integers, got %r' % (shape,))
        if len(shape) != 2 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 for n in shape):
            raise ValueError('shape: expected two non-negative integers, got %r' % (shape,))
    nx, ny = int(shape[0]), int(shape[1])
    if nx * ny >= LIMIT:
        raise ValueError('a grid of %d x %d pixels: nx * ny at most 2^31 - 1 (use a larger pixel_size, or rasterise tiles)' % (nx, ny))
    return p, origin, (nx, ny)


def raster_surface(surface):
    if surface not in SURFACES:
        raise ValueError("surface must be 'top' or 'bottom', got %r" % (surface,))
    return surface


def sun_vector(azimuth=315.0, altitude=45.0):
    """[3] fp64 numpy: the unit vector to the sun in the raster's frame (x = axes[0], y = axes[1], z = up); azimuth in degrees clockwise
    from +y, altitude in degrees above the horizon."""
    try:
        az, alt = np.float64(azimuth), np.float64(altitude)
    except (TypeError, ValueError):
        raise ValueError('hillshade: expected two numbers, got %r, %r' % (azimuth, altitude))
    if not (np.isfinite(az) and np.isfinite(alt)):
        raise ValueError('hillshade: expected finite angles, got %r, %r' % (azimuth, altitude))
    az, alt = np.deg2rad(az), np.deg2rad(alt)
    return np.array([np.sin(az) * np.cos(alt), np.cos(az) * np.cos(alt), np.sin(alt)], dtype=np.float64)


def _attr(attr, nv, dev):
    a = attr.detach() if isinstance(attr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(attr)))
    if not a.dtype.is_floating_point:
        raise ValueError('attr: expected floating-point values, got %s' % a.dtype)
    if a.dim() != 2 or a.shape[0] != nv:
        raise ValueError('attr: shape %s for %d vertices' % (tuple(a.shape), nv))
    if a.dtype not in (torch.float32, torch.float64):
        a = a.to(torch.float32)
    return a.to(dev).contiguous()


# ---- stages (nksr_amd/tools/prof_mesh_raster.py times them one by one) --------------------------------------------------------------
class Grid:
    """What every kernel takes of the grid: axes, origin, pixel size, shape."""

    def __init__(self, ax, ay, origin, p, shape):
        self.ax, self.ay, self.origin, self.p, self.shape = ax, ay, origin, p, shape

    @property
    def args(self):
        return self.ax, self.ay, self.origin[0], self.origin[1], self.p, self.shape[0], self.shape[1]


def face_boxes(x, f, g):
    """(face_valid [F] uint8, box [F, 4] int32, cand_start [F + 1] int64)."""
    nf, dev = f.shape[0], f.device
    valid = torch.empty(nf, dtype=torch.uint8, device=dev)
    box = torch.empty((nf, 4), dtype=torch.int32, device=dev)
    count = torch.empty(nf + 1, dtype=torch.int64, device=dev)
    call('nksr_raster_boxes', ptr(x), int(x.dtype == torch.float64), x.shape[0], ptr(f), is64(f), nf, *g.args, ptr(valid), ptr(box), ptr(count), stream())
    return valid, box, ops.exclusive_sum_i64(count)


def cover_candidates(x, f, g, box, cand_start, n_cand):
    """(flag [n_cand] uint8, zf [n_cand] fp64)."""
    flag = torch.empty(n_cand, dtype=torch.uint8, device=f.device)
    zf = torch.empty(n_cand, dtype=torch.float64, device=f.device)
    call('nksr_raster_test', ptr(x), int(x.dtype == torch.float64), x.shape[0], ptr(f), is64(f), f.shape[0], *g.args, ptr(box), ptr(cand_start), n_cand,
         ptr(flag), ptr(zf), stream())
    return flag, zf


def flag_starts(flag):
    """[B + 1] int64: the exclusive scan of the set flags per block of RASTER_BLOCK candidates; its last entry is the hit count."""
    n = flag.shape[0]
    counts = torch.empty((n + RASTER_BLOCK - 1) // RASTER_BLOCK + 1, dtype=torch.int64, device=flag.device)
    call('nksr_raster_flag_counts', ptr(flag), n, ptr(counts), stream())
    return ops.exclusive_sum_i64(counts)


def compact_hits(flag, zf, box, cand_start, g, block_start, n_hits):
    """(hit_pixel [H] int64, hit_face [H] int32, hit_z [H] fp64) in candidate order."""
    dev = flag.device
    pixel = torch.empty(n_hits, dtype=torch.int64, device=dev)
    face = torch.empty(n_hits, dtype=torch.int32, device=dev)
    z = torch.empty(n_hits, dtype=torch.float64, device=dev)
    call('nksr_raster_compact', ptr(flag), ptr(zf), ptr(box), ptr(cand_start), box.shape[0], flag.shape[0], g.shape[0], g.shape[1], ptr(block_start), n_hits,
         ptr(pixel), ptr(face), ptr(z), stream())
    return pixel, face, z


def sort_hits(hit_pixel, n_pixels):
    """(n_runs, run_start [R + 1] int32, run_keys [R] int64, order [H] int32, pixel_start [n_pixels + 1] int64): the hits stably sorted
    by pixel and their run table."""
    n, dev = hit_pixel.shape[0], hit_pixel.device
    ks, order = ops.sort_pairs(hit_pixel, torch.arange(n, dtype=torch.int32, device=dev), end_bit=max((n_pixels - 1).bit_length(), 1))
    nr, run_start, run_keys, _ = ops.sorted_runs(ks, keys=True)
    pixel_start = torch.empty(n_pixels + 1, dtype=torch.int64, device=dev)
    call('nksr_raster_pixel_start', ptr(run_keys), ptr(run_start), nr, n, n_pixels, ptr(pixel_start), stream())
    return nr, run_start, run_keys, order, pixel_start


def reduce_runs(nr, run_start, run_keys, order, hit_face, hit_z, bottom, shape):
    """(height [nx, ny] fp64, face, count [nx, ny] int32, layer_face [H] int32, layer_height [H] fp64)."""
    dev, n, npix = hit_face.device, hit_face.shape[0], shape[0] * shape[1]
    height = torch.full(shape, math.nan, dtype=torch.float64, device=dev)
    face = torch.full(shape, -1, dtype=torch.int32, device=dev)
    count = torch.zeros(shape, dtype=torch.int32, device=dev)
    layer_face = torch.empty(n, dtype=torch.int32, device=dev)
    layer_height = torch.empty(n, dtype=torch.float64, device=dev)
    call('nksr_raster_reduce', ptr(run_keys), ptr(run_start), nr, ptr(order), ptr(hit_face), ptr(hit_z), n, int(bottom), npix, ptr(layer_face),
         ptr(layer_height), ptr(height), ptr(face), ptr(count), stream())
    return height, face, count, layer_face, layer_height


class HeightMap:
    """The result of ``MeshRasterizer.height_map``: device tensors.  height [nx, ny] fp64 (NaN where no face covers the centre), face
    [nx, ny] int32 (the face that gives the height, -1 where none), count [nx, ny] int32 (the faces that cover the centre), valid =
    count > 0.  origin (two floats), pixel_size, shape = (nx, ny), axes, up, surface, n_faces, n_dropped (invalid faces), n_candidates,
    n_hits (all coverings)."""

    def __init__(self, rasterizer, grid, **kw):
        self._r, self._g = rasterizer, grid
        self.__dict__.update(kw)
        self._gradient = None

    @property
    def valid(self):
        return self.count > 0

    def layers(self):
        """(pixel_start [nx ny + 1] int64, layer_face [L] int32, layer_height [L] fp64): every covering; those of pixel i ny + j are
        [pixel_start[k], pixel_start[k + 1]) in ascending face id."""
        return self.pixel_start, self.layer_face, self.layer_height

    def sample(self, attr=None):
        """[nx, ny, C] fp64: ``attr`` [V, C] (default: the rasteriser's) interpolated at the hit of ``face``, NaN where empty."""
        r, g = self._r, self._g
        a = r.attr if attr is None else _attr(attr, r.n_vertices, r.device)
        if a is None:
            raise ValueError('sample: the rasteriser has no attributes, pass attr')
        out = torch.empty(self.shape + (a.shape[1],), dtype=torch.float64, device=r.device)
        call('nksr_raster_sample', ptr(r.x), int(r.x.dtype == torch.float64), r.n_vertices, ptr(r.f), is64(r.f), r.n_faces, *g.args, ptr(self.face),
             ptr(a), int(a.dtype == torch.float64), a.shape[1], ptr(out), stream())
        return out

    def _horn(self, sun):
        gx, gy, shade = (torch.empty(self.shape, dtype=torch.float64, device=self._r.device) for _ in range(3))
        call('nksr_raster_horn', ptr(self.height), self.shape[0], self.shape[1], self.pixel_size, (C.c_double * 3)(*[float(s) for s in sun]), ptr(gx),
             ptr(gy), ptr(shade), stream())
        return gx, gy, shade

    def gradient(self):
        """(gx, gy) fp64 [nx, ny]: Horn's 3 x 3 differences along axes[0] and axes[1], NaN on the rim and beside an empty pixel."""
        if self._gradient is None:
            self._gradient = self._horn((0.0, 0.0, 1.0))[:2]
        return self._gradient

    def slope(self):
        """[nx, ny] fp64: atan(hypot(gx, gy)), the angle of the surface against the horizontal in radians."""
        gx, gy = self.gradient()
        return torch.atan(torch.hypot(gx, gy))

    def hillshade(self, azimuth=315.0, altitude=45.0):
        """[nx, ny] fp64 in [0, 1]: the cosine between the surface normal and the sun (``sun_vector``), NaN where the gradient is."""
        return self._horn(sun_vector(azimuth, altitude))[2]


class MeshRasterizer:
    """Rasterisation of one triangle mesh (v [V, 3], f [F, 3] int32 / int64, attr [V, C]) on the GPU; see the module's docstring."""

    def __init__(self, v, f, attr=None, device=None):
        dev = gpu_device(device, like=v)
        vv = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
        rows3(vv, 'vertices')
        if vv.dtype not in (torch.float32, torch.float64):
            vv = vv.to(torch.float32)
        ff = mesh_input.faces(f, vv.shape[0], dev, cast_float=False, check_range=False)
        if vv.shape[0] >= LIMIT:
            raise ValueError('mesh rasteriser: %d vertices, at most 2^31 - 1' % vv.shape[0])
        if ff.shape[0] > TOPO_MAX_FACES:
            raise ValueError('mesh rasteriser: %d faces, at most 2^30' % ff.shape[0])
        self.device = dev
        self.x, self.f = vv.to(dev).contiguous(), ff            # what the kernels read
        self.n_vertices, self.n_faces = int(vv.shape[0]), int(ff.shape[0])
        self.attr = None if attr is None else _attr(attr, self.n_vertices, dev)
        self._extent = None

    def extent(self):
        """[3, 2] fp64 numpy (min, max per coordinate) over the referenced vertices of the valid faces, or None without one (one host
        read, kept)."""
        if self._extent is None:
            f = self.f.long()
            ok = ((f >= 0) & (f < self.n_vertices)).all(1) if self.n_faces else torch.zeros(0, dtype=torch.bool, device=self.device)
            if self.n_vertices:
                finite = torch.isfinite(self.x).all(1)
                ok = ok & finite[f.clamp(0, self.n_vertices - 1)].all(1)
            if self.n_faces and self.n_vertices:
                corners = self.x[f.clamp(0, self.n_vertices - 1)].to(torch.float64)                 # [F, 3, 3]
                big = corners.new_full((), math.inf)
                lo = torch.where(ok[:, None, None], corners, big).amin((0, 1))
                hi = torch.where(ok[:, None, None], corners, -big).amax((0, 1))
                self._extent = torch.stack([lo, hi], 1).cpu().numpy()
            else:
                self._extent = np.stack([np.full(3, np.inf), np.full(3, -np.inf)], 1)
        return None if not np.all(np.isfinite(self._extent)) else self._extent

    def height_map(self, pixel_size, origin=None, shape=None, axes=(0, 1), surface='top', _mark=None):
        """``HeightMap`` of the mesh seen along the axis that ``axes`` leaves out, on the grid of ``pixel_size`` whose pixel (0, 0) has
        its low corner at ``origin`` (default: the lattice point at or below the mesh's minimum) and ``shape`` = (nx, ny) pixels
        (default: up to the mesh's maximum).  ValueError for a pixel size that is not positive and finite or lies below 2^-40 of the
        largest coordinate, for nx ny >= 2^31, for a bad ``surface`` or ``axes``, and for 2^31 or more candidates.  (``_mark(stage)``
        is called after every stage of STAGES: the profiler's hook.)"""
        mark = _mark or (lambda stage: None)
        ax, ay, up = raster_axes(axes)
        surface = raster_surface(surface)
        ext = self.extent()
        p, origin, (nx, ny) = raster_grid(pixel_size, origin, shape, None if ext is None else (ext[ax, 0], ext[ax, 1], ext[ay, 0], ext[ay, 1]))
        g = Grid(ax, ay, origin, p, (nx, ny))
        valid, box, cand_start = face_boxes(self.x, self.f, g)
        n_cand, n_valid = (int(c) for c in torch.stack([cand_start[-1], valid.sum()]).tolist())
        if n_cand >= LIMIT:
            raise ValueError('mesh rasteriser: %d candidate (face, pixel) pairs, at most 2^31 - 1 (rasterise tiles)' % n_cand)
        mark('boxes')
        flag, zf = cover_candidates(self.x, self.f, g, box, cand_start, n_cand)
        mark('test')
        block_start = flag_starts(flag)
        n_hits = int(block_start[-1].item())
        hit_pixel, hit_face, hit_z = compact_hits(flag, zf, box, cand_start, g, block_start, n_hits)
        mark('compact')
        nr, run_start, run_keys, order, pixel_start = sort_hits(hit_pixel, nx * ny)
        mark('sort')
        height, face, count, layer_face, layer_height = reduce_runs(nr, run_start, run_keys, order, hit_face, hit_z, surface == 'bottom', (nx, ny))
        mark('reduce')
        return HeightMap(self, g, height=height, face=face, count=count, pixel_start=pixel_start, layer_face=layer_face, layer_height=layer_height,
                         origin=origin, pixel_size=p, shape=(nx, ny), axes=(ax, ay), up=up, surface=surface, n_faces=self.n_faces,
                         n_dropped=self.n_faces - n_valid, n_candidates=n_cand, n_hits=n_hits)
