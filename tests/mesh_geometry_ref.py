"""numpy / scipy fp64 restatement of nksr_amd/mesh_geometry.py (csrc/meshgeom.hip), written from the definitions and not from the
kernels: adjacency from the restated edge table (tests/mesh_topology_ref.py), every per-vertex sum by np.add.at or a scipy sparse
product, smoothing as x + w (D^-1 A x - x) with a 0 / 1 sparse matrix A.  Positions are taken in the precision they come in and
turned into fp64 before anything is computed."""
import numpy as np
from scipy.sparse import coo_matrix, csr_matrix

import mesh_topology_ref as T

INTERIOR, ON_BOUNDARY, UNREFERENCED = 0, 1, 2


def adjacency(f, nv):
    """neighbour_start [V + 1], neighbours [2E] (rows ascending), neighbour_edge, neighbour_class, degree [V], vertex_kind [V]."""
    t = T.edge_table(f, nv)
    e = t['edges'].astype(np.int64).reshape(-1, 2)
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    eid = np.concatenate([np.arange(len(e)), np.arange(len(e))])
    o = np.lexsort((dst, src))
    src, dst, eid = src[o], dst[o], eid[o]
    degree = np.bincount(src, minlength=nv).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(degree)])
    kind = np.where(t['vertex_ref'], INTERIOR, UNREFERENCED).astype(np.uint8)
    on_border = e[t['edge_classes'] == T.BOUNDARY].reshape(-1)
    kind[on_border] = ON_BOUNDARY
    return {'neighbour_start': start, 'neighbours': dst.astype(np.int32), 'neighbour_edge': eid.astype(np.int32),
            'neighbour_class': t['edge_classes'][eid] if len(e) else np.zeros(0, np.uint8), 'vertex_degree': degree, 'vertex_kind': kind,
            'source': src, 'table': t}


def face_quantities(v, f):
    """Of the VALID faces: their vertex indices [Fv, 3], corner angles, cotangents [Fv, 3], unit normals [Fv, 3], areas [Fv]."""
    x = np.asarray(v).astype(np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    g = f[T.valid_faces(f, len(x))]
    p = x[g]                                                            # [Fv, 3 corners, 3 axes]
    e1, e2 = np.roll(p, -1, axis=1) - p, np.roll(p, -2, axis=1) - p     # the two edges leaving every corner
    s, d = np.linalg.norm(np.cross(e1, e2), axis=2), (e1 * e2).sum(2)
    with np.errstate(divide='ignore', invalid='ignore'):
        cot = d / s
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    unit = np.divide(n, length[:, None], out=np.zeros_like(n), where=length[:, None] > 0)
    return g, np.arctan2(s, d), cot, unit, 0.5 * length


def vertex_normals(v, f, weighting='angle'):
    """[V, 3] fp64 unit normals, zero rows where the sum vanishes."""
    g, angle, _, unit, area = face_quantities(v, f)
    w = angle if weighting == 'angle' else np.repeat(area[:, None], 3, 1)
    n = np.zeros((len(v), 3))
    np.add.at(n, g.reshape(-1), (w[:, :, None] * unit[:, None, :]).reshape(-1, 3))
    length = np.linalg.norm(n, axis=1)
    return np.divide(n, length[:, None], out=np.zeros_like(n), where=length[:, None] > 0)


def vertex_areas(v, f):
    g, _, _, _, area = face_quantities(v, f)
    a = np.zeros(len(v))
    np.add.at(a, g.reshape(-1), np.repeat(area / 3.0, 3))
    return a


def _undefined(v, f):
    return (adjacency(f, len(v))['vertex_kind'] != INTERIOR) | ~(vertex_areas(v, f) > 0)


def gaussian_curvature(v, f, integrated=False):
    g, angle, _, _, _ = face_quantities(v, f)
    s = np.zeros(len(v))
    np.add.at(s, g.reshape(-1), angle.reshape(-1))
    k = 2.0 * np.pi - s
    if not integrated:
        with np.errstate(divide='ignore', invalid='ignore'):
            k = k / vertex_areas(v, f)
    return np.where(_undefined(v, f), np.nan, k)


def cotangent_matrix(v, f):
    """Sparse symmetric W [V, V]: W_ij = the sum over all valid faces on edge (i, j) of the cotangent of the opposite corner."""
    g, _, cot, _, _ = face_quantities(v, f)
    i, j = np.roll(g, -1, axis=1).reshape(-1), np.roll(g, -2, axis=1).reshape(-1)       # corner k is opposite the edge (k + 1, k + 2)
    w = cot.reshape(-1)
    nv = len(v)
    return coo_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(nv, nv)).tocsr()


def weighted_laplacian(v, f):
    """[V, 3]: sum_j w_ij (x_j - x_i) = 2 A_i Delta x_i, without the division."""
    x = np.asarray(v).astype(np.float64)
    w = cotangent_matrix(v, f).tocoo()                                  # (differences first: w @ x - rowsum x would cancel |w x| >> the result)
    out = np.zeros((len(x), 3))
    np.add.at(out, w.row, w.data[:, None] * (x[w.col] - x[w.row]))
    return out


def mean_curvature(v, f):
    a = vertex_areas(v, f)
    with np.errstate(divide='ignore', invalid='ignore'):
        lap = weighted_laplacian(v, f) / (2.0 * a[:, None])
        h = 0.5 * np.linalg.norm(lap, axis=1) * np.sign(-(lap * vertex_normals(v, f, 'angle')).sum(1))
    return np.where(_undefined(v, f), np.nan, h)


def smooth(v, f, iterations, method='taubin', lam=0.5, mu=-0.53, boundary='fixed', fixed=None):
    """fp64 positions after the steps (the caller rounds)."""
    x = np.asarray(v).astype(np.float64)
    nv = len(x)
    a = adjacency(f, nv)
    src, dst, kind = a['source'], a['neighbours'].astype(np.int64), a['vertex_kind']
    use = np.ones(len(src), bool)
    if boundary == 'curve':
        use = (kind[src] != ON_BOUNDARY) | (a['neighbour_class'] == T.BOUNDARY)
    m = csr_matrix((np.ones(int(use.sum())), (src[use], dst[use])), shape=(nv, nv))
    count = np.asarray(m.sum(1)).reshape(-1)
    moves = (kind != UNREFERENCED) & (count > 0)
    if boundary == 'fixed':
        moves &= kind != ON_BOUNDARY
    if fixed is not None:
        moves &= ~np.asarray(fixed, bool)
    weights = [lam, mu] * iterations if method == 'taubin' else [lam] * iterations
    for w in weights:
        mean = (m @ x) / np.maximum(count, 1)[:, None]
        x = np.where(moves[:, None], x + w * (mean - x), x)
    return x


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def noisy(v, sigma, seed=0):
    """fp32 vertices with normal noise of standard deviation sigma."""
    return (np.asarray(v, np.float64) + np.random.RandomState(seed).normal(0, sigma, np.shape(v))).astype(np.float32)


def holed_sphere():
    """uv_sphere(64, 32) without the ten faces RandomState(0) picks."""
    v, f = T.uv_sphere(64, 32)
    return v, np.delete(f, np.random.RandomState(0).choice(len(f), 10, replace=False), 0)
