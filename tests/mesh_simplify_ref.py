"""numpy fp64 restatement of nksr_amd/mesh_simplify.py (csrc/meshsimp.hip), written from the definitions of DESIGN.md section 3.14 and
not from the kernels: cells by np.floor of an fp64 subtraction and division, clusters by np.unique, every per-cluster sum by np.add.at,
the 3 x 3 systems by np.linalg.solve, the duplicate faces by np.unique over the sorted id triples.  Plus the rotated cube the tests
share and the host replay of the target-size bisection."""
import math

import numpy as np

import mesh_topology_ref as T

MAX_INDEX = 1 << 21


def referenced(f, nv):
    """(valid [F] bool, referenced [V] bool)."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = T.valid_faces(f, nv)
    ref = np.zeros(nv, bool)
    ref[f[ok].reshape(-1)] = True
    return ok, ref


def grid(v, f, cell_size, origin=None):
    """(origin [3] fp64, cell index [V, 3] int64 with -1 rows for unreferenced vertices); the ValueErrors of the definition."""
    x = np.asarray(v).astype(np.float64).reshape(-1, 3)
    _, ref = referenced(f, len(x))
    if not np.isfinite(x[ref]).all():
        raise ValueError('non-finite coordinates')
    idx = np.full((len(x), 3), -1, np.int64)
    if not ref.any():
        return np.zeros(3) if origin is None else np.asarray(origin, np.float64), idx
    lo = x[ref].min(0)
    if origin is None:
        origin = lo
    origin = np.asarray(origin, np.float64).reshape(3)
    if (origin > lo).any():
        raise ValueError('origin above the minimum')
    idx[ref] = np.floor((x[ref] - origin) / np.float64(cell_size)).astype(np.int64)         # a subtraction, then a division
    if idx.max() >= MAX_INDEX:
        raise ValueError('extent %d' % idx.max())
    return origin, idx


def clusters(v, f, cell_size, origin=None):
    """(origin, cluster id [V] (-1: unreferenced), keys [K] ascending)."""
    origin, idx = grid(v, f, cell_size, origin)
    ref = idx[:, 0] >= 0
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    uk, inv = np.unique(key[ref], return_inverse=True)
    cid = np.full(len(idx), -1, np.int64)
    cid[ref] = inv.reshape(-1)
    return origin, cid, uk


def map_faces(f, nv, cid, dedup=True):
    """(cluster triples [F, 3], keep [F] bool, invalid, collapsed, duplicate counts)."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = T.valid_faces(f, nv)
    g = np.where(ok[:, None], cid[np.where(ok[:, None], f, 0)] if nv else 0, 0).reshape(-1, 3)
    collapsed = ok & ((g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2]))
    keep = ok & ~collapsed
    dup = 0
    if dedup and keep.any():
        alive = np.nonzero(keep)[0]
        _, first = np.unique(np.sort(g[alive], axis=1), axis=0, return_index=True)     # (the first occurrence: the lowest face index)
        keep = np.zeros(len(f), bool)
        keep[alive[first]] = True
        dup = len(alive) - len(first)
    return g, keep, int((~ok).sum()), int(collapsed.sum()), dup


def count_faces(v, f, cell_size, origin=None, dedup=True):
    _, cid, _ = clusters(v, f, cell_size, origin)
    return int(map_faces(f, len(np.asarray(v).reshape(-1, 3)), cid, dedup)[1].sum())


def representatives(v, f, cell_size, origin, cid, keys, placement='quadric', regularisation=1e-3):
    """[K, 3] fp64 representative of every cluster, in ascending key order."""
    x = np.asarray(v).astype(np.float64).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    nk, h = len(keys), np.float64(cell_size)
    cell = np.stack([keys >> 42, (keys >> 21) & (MAX_INDEX - 1), keys & (MAX_INDEX - 1)], 1)
    centre = origin + (cell + 0.5) * h
    ref = cid >= 0
    s = np.zeros((nk, 3))
    np.add.at(s, cid[ref], x[ref] - centre[cid[ref]])
    mean = s / np.maximum(np.bincount(cid[ref], minlength=nk), 1)[:, None]
    if placement == 'mean':
        return centre + mean
    g = f[T.valid_faces(f, len(x))]
    p = x[g]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    has_area = length > 0
    g, p, n, length = g[has_area], p[has_area], n[has_area], length[has_area]
    unit, area = n / length[:, None], 0.5 * length
    a_mat, b_vec = np.zeros((nk, 3, 3)), np.zeros((nk, 3))
    for k in range(3):                                                  # once per corner, also for two or three corners in one cluster
        c = cid[g[:, k]]
        d = -(unit * (p[:, 0] - centre[c])).sum(1)
        np.add.at(a_mat, c, area[:, None, None] * unit[:, :, None] * unit[:, None, :])
        np.add.at(b_vec, c, (area * d)[:, None] * unit)
    tau = np.trace(a_mat, axis1=1, axis2=2)
    out = mean.copy()
    for c in np.nonzero(tau > 0)[0]:
        m = a_mat[c] + regularisation * tau[c] * np.eye(3)
        out[c] = np.linalg.solve(m, -b_vec[c] + regularisation * tau[c] * mean[c])
    return centre + np.clip(out, -0.5 * h, 0.5 * h)


def simplify(v, f, cell_size, colors=None, origin=None, placement='quadric', regularisation=1e-3, dedup=True):
    """The whole definition; a dict with the fields of the result object plus 'cluster_id' [V], 'representatives' [K, 3] fp64 (every
    cluster, before those no face names are dropped), 'cluster_kept' [K] bool and 'v2_f64'."""
    v = np.asarray(v).reshape(-1, 3)
    f = np.asarray(f).reshape(-1, 3)
    nv = len(v)
    origin, cid, keys = clusters(v, f, cell_size, origin)
    g, keep, invalid, collapsed, dup = map_faces(f, nv, cid, dedup)
    rep = representatives(v, f, cell_size, origin, cid, keys, placement, regularisation)
    used = np.zeros(len(keys), bool)
    used[g[keep].reshape(-1)] = True
    new = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    out = {'cluster_id': cid, 'n_clusters': len(keys), 'invalid_faces': invalid, 'collapsed_faces': collapsed, 'duplicate_faces': dup,
           'representatives': rep, 'cluster_kept': used, 'v2_f64': rep[used], 'v2': rep[used].astype(v.dtype),
           'f2': new[g[keep]].astype(f.dtype).reshape(-1, 3), 'vertex_map': np.where(cid >= 0, new[np.maximum(cid, 0)] if len(keys) else -1, -1),
           'cell_size': float(cell_size), 'origin': origin, 'c2': None}
    if colors is not None:
        col = np.asarray(colors)
        ref = cid >= 0
        s = np.zeros((len(keys), col.shape[1]))
        np.add.at(s, cid[ref], col[ref].astype(np.float64))
        out['c2_f64'] = (s / np.maximum(np.bincount(cid[ref], minlength=len(keys)), 1)[:, None])[used]
        out['c2'] = out['c2_f64'].astype(col.dtype)
    return out


def diagonal(v, f):
    """fp64 bounding-box diagonal of the referenced vertices."""
    x = np.asarray(v).astype(np.float64).reshape(-1, 3)
    _, ref = referenced(f, len(x))
    d = x[ref].max(0) - x[ref].min(0)
    return math.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) + float(d[2]) * float(d[2]))


def target_cell_size(count, diag, target, steps=24):
    """The bisection of the definition over ``count(cell_size)``; (cell_size, steps taken)."""
    lo, hi = diag / 2.0 ** 20, 2.0 * diag
    if count(lo) <= target:
        return lo, 0
    for _ in range(steps):
        mid = math.sqrt(lo * hi)
        if count(mid) > target:
            lo = mid
        else:
            hi = mid
    return hi, steps


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
CUBE_SIDE = 12


def rotation():
    """0.3 rad about z after 0.2 rad about x."""
    cx, sx, cz, sz = math.cos(0.2), math.sin(0.2), math.cos(0.3), math.sin(0.3)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ rx


def rotated_cube(offset=0.0):
    """The surface of a 12^3 block of unit voxels, rotated off the grid axes; (v fp64 [866, 3], f int64 [1728, 3])."""
    n = CUBE_SIDE
    v, f = T.voxel_mesh({(x, y, z) for x in range(n) for y in range(n) for z in range(n)}, 0)
    return v.astype(np.float64) @ rotation().T + offset, f


def cube_corners(offset=0.0):
    n = CUBE_SIDE
    c = np.array([[x, y, z] for x in (0, n) for y in (0, n) for z in (0, n)], np.float64)
    return c @ rotation().T + offset


def corner_error(v2, offset=0.0):
    """The worst distance from a corner of the cube to the nearest vertex of v2."""
    d = np.linalg.norm(cube_corners(offset)[:, None, :] - np.asarray(v2, np.float64)[None, :, :], axis=2)
    return float(d.min(1).max())


def plane_error(v2, offset=0.0):
    """The worst distance of a vertex of v2 to the nearest of the cube's six planes."""
    local = (np.asarray(v2, np.float64) - offset) @ rotation()           # back into the cube's axes
    d = np.minimum(np.abs(local), np.abs(local - CUBE_SIDE))
    return float(d.min(1).max())


def closed_manifold_oriented(f, nv):
    t = T.edge_table(f, nv)
    return t['boundary_edges'] == 0 and t['nonmanifold_edges'] == 0 and t['misoriented_edges'] == 0, t['euler']
