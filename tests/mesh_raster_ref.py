"""Numpy restatement of the mesh rasteriser (nksr_amd/mesh_raster.py, csrc/meshraster.hip): the same operations
in the same order, every product and sum rounded on its own, as a brute force over every (face, pixel) pair.  It has no candidate
boxes, so a comparison against it also checks that the GPU's boxes are conservative.  Plain fp64 numpy, one face at a time over the
whole grid; meant for the small shapes of the tests."""
import math

import numpy as np


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def frame(v, axes):
    """(x, y, z) fp64 [V]: the caller's values widened exactly (fp32 stays fp32-valued; anything else is read as fp32, as the GPU does)."""
    v = np.asarray(v)
    if v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float32)
    up = 3 - axes[0] - axes[1]
    return v[:, axes[0]].astype(np.float64), v[:, axes[1]].astype(np.float64), v[:, up].astype(np.float64)


def valid_faces(v, f):
    """[F] bool: every index inside [0, V) and every corner finite."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    if len(v):
        ok &= np.isfinite(v).all(1)[np.clip(f, 0, len(v) - 1)].all(1)
    return ok


def grid(v, f, pixel_size, origin, shape, axes):
    """(p, origin, shape): ``origin=None`` is floor(min / p) p over the referenced vertices of the valid faces, ``shape=None``
    floor((max - origin) / p) + 1 per axis; (0, 0) and an empty grid without a valid face."""
    p = float(pixel_size)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ref = f[valid_faces(v, f)].reshape(-1)
    x, y, _ = frame(v, axes)
    if origin is None:
        origin = (math.floor(x[ref].min() / p) * p, math.floor(y[ref].min() / p) * p) if len(ref) else (0.0, 0.0)
    origin = (float(origin[0]), float(origin[1]))
    if shape is None:
        shape = (max(math.floor((x[ref].max() - origin[0]) / p) + 1, 0), max(math.floor((y[ref].max() - origin[1]) / p) + 1, 0)) if len(ref) else (0, 0)
    return p, origin, (int(shape[0]), int(shape[1]))


def centres(origin, p, n):
    """[n] fp64: origin + (k + 0.5) p, one rounded product and one rounded sum."""
    return origin + (np.arange(n, dtype=np.float64) + 0.5) * p


def edge(px, py, qx, qy):
    """(e, s): the edge function Px Qy - Py Qx and its sign with the tie-break."""
    e = px * qy - py * qx
    tie = np.where(py != qy, np.where(py > qy, 1, -1), np.where(qx != px, np.where(qx > px, 1, -1), 0))
    return e, np.where(e > 0, 1, np.where(e < 0, -1, tie))


def cover(xa, ya, xb, yb, xc, yc, X, Y):
    """(covered, U, V, W, det) of the face with corners a, b, c at the centres (X, Y) (arrays that broadcast)."""
    Ax, Ay, Bx, By, Cx, Cy = xa - X, ya - Y, xb - X, yb - Y, xc - X, yc - Y
    U, su = edge(Bx, By, Cx, Cy)
    V, sv = edge(Cx, Cy, Ax, Ay)
    W, sw = edge(Ax, Ay, Bx, By)
    det = (U + V) + W
    return (su != 0) & (su == sv) & (su == sw) & (det != 0), U, V, W, det


def height_map(v, f, pixel_size, origin=None, shape=None, axes=(0, 1), surface='top'):
    """dict: height [nx, ny] fp64, face / count [nx, ny] int32, pixel_start [nx ny + 1] int64, layer_face [L] int32, layer_height [L]
    fp64, origin, pixel_size, shape, axes, n_dropped, n_hits."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    p, origin, (nx, ny) = grid(v, f, pixel_size, origin, shape, axes)
    x, y, z = frame(v, axes)
    ok = valid_faces(v, f)
    X, Y = centres(origin[0], p, nx)[:, None], centres(origin[1], p, ny)[None, :]
    height = np.full((nx, ny), np.nan)
    face = np.full((nx, ny), -1, np.int32)
    count = np.zeros((nx, ny), np.int32)
    hits_pixel, hits_face, hits_z = [], [], []
    with np.errstate(all='ignore'):
        for k in np.nonzero(ok)[0]:
            a, b, c = f[k]
            covered, U, V, W, det = cover(x[a], y[a], x[b], y[b], x[c], y[c], X, Y)
            if not covered.any():
                continue
            zf = ((U * z[a] + V * z[b]) + W * z[c]) / det
            better = covered & ((count == 0) | (zf < height if surface == 'bottom' else zf > height))      # strictly: the lowest face id keeps a tie
            height[better] = zf[better]
            face[better] = k
            count += covered
            pix = np.nonzero(covered.reshape(-1))[0]
            hits_pixel.append(pix)
            hits_face.append(np.full(len(pix), k, np.int32))
            hits_z.append(zf.reshape(-1)[pix])
    hp = np.concatenate(hits_pixel) if hits_pixel else np.zeros(0, np.int64)
    hf = np.concatenate(hits_face) if hits_face else np.zeros(0, np.int32)
    hz = np.concatenate(hits_z) if hits_z else np.zeros(0, np.float64)
    order = np.argsort(hp, kind='stable')                   # per pixel in ascending face id
    pixel_start = np.concatenate([[0], np.cumsum(np.bincount(hp, minlength=nx * ny))]).astype(np.int64)
    return dict(height=height, face=face, count=count, pixel_start=pixel_start, layer_face=hf[order], layer_height=hz[order], origin=origin,
                pixel_size=p, shape=(nx, ny), axes=tuple(axes), n_dropped=int((~ok).sum()), n_hits=len(hp))


def sample(v, f, hm, attr):
    """[nx, ny, C] fp64: attr interpolated at the hit of hm['face'], U, V, W recomputed by the same operations; NaN where empty."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    attr = np.asarray(attr)
    t = attr.astype(np.float64) if attr.dtype in (np.float32, np.float64) else attr.astype(np.float32).astype(np.float64)
    nx, ny = hm['shape']
    x, y, _ = frame(v, hm['axes'])
    X = np.broadcast_to(centres(hm['origin'][0], hm['pixel_size'], nx)[:, None], (nx, ny))
    Y = np.broadcast_to(centres(hm['origin'][1], hm['pixel_size'], ny)[None, :], (nx, ny))
    out = np.full((nx, ny, t.shape[1]), np.nan)
    hit = hm['face'] >= 0
    a, b, c = f[hm['face'][hit]].T
    _, U, V, W, det = cover(x[a], y[a], x[b], y[b], x[c], y[c], X[hit], Y[hit])
    out[hit] = ((U[:, None] * t[a] + V[:, None] * t[b]) + W[:, None] * t[c]) / det[:, None]
    return out


def gradient(h, p):
    """(gx, gy) [nx, ny]: Horn's 3 x 3 differences, NaN on the rim and where one of the nine heights is not finite."""
    h = np.asarray(h, np.float64)
    gx, gy = np.full(h.shape, np.nan), np.full(h.shape, np.nan)
    if h.shape[0] < 3 or h.shape[1] < 3:
        return gx, gy

    def at(di, dj):
        return h[1 + di:h.shape[0] - 1 + di, 1 + dj:h.shape[1] - 1 + dj]
    ok = np.ones((h.shape[0] - 2, h.shape[1] - 2), bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ok &= np.isfinite(at(di, dj))
    scale = 8.0 * p
    with np.errstate(all='ignore'):
        x = (((at(1, -1) + 2.0 * at(1, 0)) + at(1, 1)) - ((at(-1, -1) + 2.0 * at(-1, 0)) + at(-1, 1))) / scale
        y = (((at(-1, 1) + 2.0 * at(0, 1)) + at(1, 1)) - ((at(-1, -1) + 2.0 * at(0, -1)) + at(1, -1))) / scale
    gx[1:-1, 1:-1] = np.where(ok, x, np.nan)
    gy[1:-1, 1:-1] = np.where(ok, y, np.nan)
    return gx, gy


def sun(azimuth, altitude):
    az, alt = np.deg2rad(np.float64(azimuth)), np.deg2rad(np.float64(altitude))
    return np.array([np.sin(az) * np.cos(alt), np.cos(az) * np.cos(alt), np.sin(alt)], dtype=np.float64)


def hillshade(h, p, azimuth=315.0, altitude=45.0):
    gx, gy = gradient(h, p)
    sx, sy, sz = sun(azimuth, altitude)
    with np.errstate(all='ignore'):
        t = (sz - (sx * gx + sy * gy)) / np.sqrt((1.0 + gx * gx) + gy * gy)
    return np.where(np.isnan(gx), np.nan, np.where(t > 0.0, t, 0.0))


# ---- meshes of the tests ------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=2, radius=1.0):
    """(v [V, 3] fp64, f [F, 3] int64): 20 * 4^subdivisions outward faces."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v) * radius, np.array(f, np.int64)


def snapped_icosphere(pixel=1.0, radius=11.0, offset=0.0, dtype=np.float64):
    """The twice-subdivided icosphere with x and y snapped to half pixels: vertices and edges lie exactly under pixel centres."""
    v, f = icosphere(2, radius)
    v[:, :2] = np.round(v[:, :2] / (0.5 * pixel)) * (0.5 * pixel)
    return (v + offset).astype(dtype), f


def diagonal_square(n, pixel=1.0, mixed=False):
    """The square [0, n p]^2 at z = 0 cut along its diagonal; ``mixed``: the second triangle wound the other way."""
    s = n * pixel
    v = np.array([[0, 0, 0], [s, 0, 0], [s, s, 0], [0, s, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 2] if mixed else [0, 2, 3]], np.int64)
    return v, f


def triangle_soup(n=300, nx=37, ny=29, pixel=0.25, origin=(-3.0, -2.0), seed=3, dtype=np.float64):
    """n random triangles with x, y snapped to half pixels round a grid of nx x ny: most on it, some over the rim, every seventh wholly
    outside (no candidates); z random."""
    rng = np.random.default_rng(seed)
    half = 0.5 * pixel
    centre = np.stack([rng.integers(-4, 2 * nx + 4, n), rng.integers(-4, 2 * ny + 4, n)], 1)
    corner = centre[:, None, :] + rng.integers(-7, 8, (n, 3, 2))
    corner[::7] += np.array([4 * nx + 40, 0])
    xy = np.asarray(origin) + corner * half
    z = rng.uniform(-1.0, 1.0, (n, 3, 1))
    v = np.concatenate([xy, z], 2).reshape(-1, 3).astype(dtype)
    return v, np.arange(3 * n, dtype=np.int64).reshape(-1, 3)
