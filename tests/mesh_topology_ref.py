"""numpy / scipy restatement of nksr_amd/mesh_topology.py (csrc/meshtopo.hip): the unique-edge table by np.unique over half-edges,
connected components by scipy.sparse.csgraph relabelled to "ascending minimum node index", compaction by np.cumsum.  Plus the small
meshes the tests share."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from mesh_query_ref import torus, uv_sphere, voxel_mesh, voxel_sets  # noqa: F401  (the tests take the builders from here)

BOUNDARY, INTERIOR, MISORIENTED, NONMANIFOLD = 1, 2, 3, 4


def valid_faces(f, nv):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < nv)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def _sorted_halfedges(f, nv):
    """(key, id, forward) of the valid faces' half-edges, sorted by key, ids ascending inside a key."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = valid_faces(f, nv)
    a, b = f, np.roll(f, -1, axis=1)                                    # half-edge k: corner k -> corner k + 1
    key = ((np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1)
    ids = np.arange(3 * len(f))
    sel = np.repeat(ok, 3)
    key, ids, fwd = key[sel], ids[sel], (a < b).reshape(-1)[sel]
    o = np.argsort(key, kind='stable')
    return key[o], ids[o], fwd[o]


def edge_table(f, nv):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = valid_faces(f, nv)
    key, ids, fwd = _sorted_halfedges(f, nv)
    uk, start, count = np.unique(key, return_index=True, return_counts=True)
    cls = np.where(count == 1, BOUNDARY, np.where(count > 2, NONMANIFOLD, INTERIOR)).astype(np.uint8)
    two = np.nonzero(count == 2)[0]
    h0, h1 = ids[start[two]], ids[start[two] + 1]
    cls[two[fwd[start[two]] == fwd[start[two] + 1]]] = MISORIENTED
    adj = np.full(3 * len(f), -1, np.int32)
    adj[h0], adj[h1] = h1 // 3, h0 // 3
    ref = np.zeros(nv, bool)
    ref[f[ok].reshape(-1)] = True
    return {'edges': np.stack([uk >> 32, uk & 0xFFFFFFFF], 1).astype(np.int32).reshape(-1, 2), 'edge_counts': count.astype(np.int32),
            'edge_classes': cls, 'face_adjacency': adj.reshape(-1, 3), 'first_face': (ids[start] // 3) if len(uk) else np.zeros(0, np.int64),
            'num_edges': len(uk), 'boundary_edges': int((cls == BOUNDARY).sum()), 'nonmanifold_edges': int((cls == NONMANIFOLD).sum()),
            'misoriented_edges': int((cls == MISORIENTED).sum()), 'invalid_faces': int((~ok).sum()), 'referenced_vertices': int(ref.sum()),
            'euler': int(ref.sum()) - len(uk) + int(ok.sum()), 'vertex_ref': ref, 'face_valid': ok}


def _relabel(raw, member):
    """Dense labels of the members in the order of each component's smallest member; -1 elsewhere."""
    out = np.full(len(raw), -1, np.int32)
    idx = np.nonzero(member)[0]
    if len(idx) == 0:
        return out, 0
    u, first = np.unique(raw[idx], return_index=True)                   # first: position (in idx) of each raw label's smallest member
    rank = np.empty(len(u), np.int64)
    rank[np.argsort(first)] = np.arange(len(u))
    out[idx] = rank[np.searchsorted(u, raw[idx])]
    return out, len(u)


def face_areas(v, f, nv):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < nv)).all(1)
    g = np.where(ok[:, None], f, 0)
    p = np.asarray(v, np.float32).astype(np.float64)[g]
    a = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    return np.where(ok, a, 0.0)


def components(v, f, connectivity='edge'):
    v = np.asarray(v)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    nv, nf = len(v), len(f)
    t = edge_table(f, nv)
    ok, ref = t['face_valid'], t['vertex_ref']
    if connectivity == 'vertex':
        e = t['edges'].astype(np.int64)
        g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv))
        raw = connected_components(g, directed=False)[1] if nv else np.zeros(0, np.int64)
        vlab, n = _relabel(raw, ref)
        flab = np.where(ok, vlab[np.where(ok, f[:, 0], 0)] if nv else -1, -1).astype(np.int32)
    else:
        key, ids, _ = _sorted_halfedges(f, nv)
        same = key[1:] == key[:-1]
        a, b = ids[:-1][same] // 3, ids[1:][same] // 3
        g = coo_matrix((np.ones(len(a)), (a, b)), shape=(nf, nf))
        raw = connected_components(g, directed=False)[1] if nf else np.zeros(0, np.int64)
        flab, n = _relabel(raw, ok)
        vlab = np.full(nv, np.iinfo(np.int32).max, np.int32)
        np.minimum.at(vlab, f[ok].reshape(-1), np.repeat(flab[ok], 3))
        vlab[~ref] = -1
    out = {'n': n, 'face_label': flab, 'vertex_label': vlab}
    out['face_count'] = np.bincount(flab[ok], minlength=n).astype(np.int64)
    pairs = np.unique((np.repeat(flab[ok].astype(np.int64), 3) << 32) | f[ok].reshape(-1))      # distinct (component, vertex)
    out['vertex_count'] = np.bincount(pairs >> 32, minlength=n).astype(np.int64)
    elab = flab[t['first_face']]
    out['edge_count'] = np.bincount(elab, minlength=n).astype(np.int64)
    out['boundary_edges'] = np.bincount(elab[t['edge_classes'] == BOUNDARY], minlength=n).astype(np.int64)
    out['euler'] = out['vertex_count'] - out['edge_count'] + out['face_count']
    out['closed'] = out['boundary_edges'] == 0
    out['area'] = np.bincount(flab[ok], weights=face_areas(v, f, nv)[ok], minlength=n)
    p = np.asarray(v, np.float32)[f[ok]] + np.float32(0.0)              # [Fv, 3 corners, 3 axes]
    lo, hi = np.full((n, 3), np.inf, np.float32), np.full((n, 3), -np.inf, np.float32)
    np.minimum.at(lo, flab[ok], p.min(1))
    np.maximum.at(hi, flab[ok], p.max(1))
    out['box'] = np.concatenate([lo, hi], 1)
    return out


def compact(v, f, face_keep, colors=None):
    """(v2, f2, c2, vertex_map) of the kept valid faces: np.cumsum over the flags."""
    v, f = np.asarray(v), np.asarray(f)
    nv = len(v)
    keep = np.asarray(face_keep, bool) & valid_faces(f, nv)
    vflag = np.zeros(nv, bool)
    vflag[f[keep].reshape(-1)] = True
    vmap = np.where(vflag, np.cumsum(vflag) - 1, -1).astype(np.int64)
    f2 = vmap[f[keep]].astype(f.dtype).reshape(-1, 3)
    return v[vflag], f2, None if colors is None else np.asarray(colors)[vflag], vmap


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def three_fan():
    """Three triangles on the common edge (0, 1)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)


def cube(origin):
    return voxel_mesh({tuple(origin)}, 0)


def two_cubes_sharing_a_vertex():
    """Unit cubes at (0, 0, 0) and (1, 1, 1), the corner (1, 1, 1) welded."""
    v0, f0 = cube((0, 0, 0))
    v1, f1 = cube((1, 1, 1))
    i0 = int(np.nonzero((v0 == 1).all(1))[0][0])
    i1 = int(np.nonzero((v1 == 1).all(1))[0][0])
    remap = np.arange(len(v1)) + len(v0)
    remap[i1] = i0
    remap[i1 + 1:] -= 1
    return np.concatenate([v0, np.delete(v1, i1, 0)]), np.concatenate([f0, remap[f1]])


def tetrahedron(centre, r):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * r + np.asarray(centre, np.float64)
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)


def sphere_with_floaters(n_floaters=20, seed=0):
    """uv_sphere(64, 32) followed by small tetrahedra outside it; (v, f, colours [V, 3] float32, faces of the sphere)."""
    v, f = uv_sphere(64, 32)
    rs = np.random.RandomState(seed)
    vs, fs, n0 = [v], [f], len(f)
    for _ in range(n_floaters):
        d = rs.normal(size=3)
        tv, tf = tetrahedron(d / np.linalg.norm(d) * rs.uniform(0.6, 0.9), 0.01)
        fs.append(tf + sum(len(x) for x in vs))
        vs.append(tv)
    v, f = np.concatenate(vs), np.concatenate(fs)
    return v, f, rs.uniform(0, 1, (len(v), 3)).astype(np.float32), n0


def shuffled(v, f, seed):
    """The same mesh with vertex and face order permuted (fixed seed)."""
    rs = np.random.RandomState(seed)
    pv, pf = rs.permutation(len(v)), rs.permutation(len(f))
    inv = np.empty(len(v), np.int64)
    inv[pv] = np.arange(len(v))
    return np.asarray(v)[pv], inv[np.asarray(f)][pf]


def triangle_strip(n_faces):
    """One long path of n_faces triangles over n_faces + 2 vertices."""
    i = np.arange(n_faces)
    f = np.stack([i, i + 1, i + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    v = np.stack([(np.arange(n_faces + 2) // 2).astype(np.float32), (np.arange(n_faces + 2) % 2).astype(np.float32),
                  np.zeros(n_faces + 2, np.float32)], 1)
    return v, f.astype(np.int64)


def disjoint_triangles(n):
    f = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    rs = np.random.RandomState(3)
    return rs.uniform(-1, 1, (3 * n, 3)).astype(np.float32), f


def random_soup(n_faces, n_vertices, seed=5):
    rs = np.random.RandomState(seed)
    return rs.uniform(-1, 1, (n_vertices, 3)).astype(np.float32), rs.randint(0, n_vertices, (n_faces, 3)).astype(np.int64)
