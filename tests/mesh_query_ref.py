"""numpy restatement of the mesh queries of csrc/meshquery.hip (nksr_amd/mesh_query.py), for the tests.

``crossings`` repeats the kernel's fp32 crossing predicate operation for operation (float32 numpy arithmetic rounds every operation
once, like the kernel's code under ``fp contract(off)``): the shear, the fp32 edge functions, their fp64 recomputation at an exact 0,
the per-edge tie-break and the half-line test.  Besides it: an fp64 brute-force point-triangle distance, the fp64 generalised
winding number, and meshes whose inside is known exactly (unions of unit voxels, convex polyhedra, a UV sphere, a torus).
"""
import numpy as np

DIRS = np.array([(0.5, 0.25, 1.0), (1.0, -0.375, 0.625), (-0.625, 1.0, -0.25), (-0.25, -0.5, -1.0), (-1.0, 0.625, -0.375),
                 (0.375, -1.0, 0.5), (-0.375, 0.75, 1.0)], np.float32)          # NKSR_BVH_RAY_DIRS


def recentre(v, q=None):
    """float32 copies of v (and q) minus the float64 centre of v's bounding box, as MeshQuery takes them."""
    v = np.asarray(v, np.float64)
    c = 0.5 * (v.min(0) + v.max(0)) if len(v) else np.zeros(3)
    out = (v - c).astype(np.float32)
    return (out, (np.asarray(q, np.float64) - c).astype(np.float32)) if q is not None else out


def _frame(d):
    m = np.abs(d)
    kz = 0 if (m[0] >= m[1] and m[0] >= m[2]) else (1 if m[1] >= m[2] else 2)
    kx = 0 if kz == 2 else kz + 1
    ky = 0 if kx == 2 else kx + 1
    sz = d[kz]
    return kx, ky, kz, np.float32(d[kx] * sz), np.float32(d[ky] * sz), np.float32(sz)


def _edge_sign(px, py, qx, qy):
    """(fp32 edge function, its sign with the fp64 recomputation and the tie-break)."""
    e = px * qy - py * qx
    s = np.sign(e).astype(np.int8)
    z = s == 0
    if z.any():
        e64 = px[z].astype(np.float64) * qy[z].astype(np.float64) - py[z].astype(np.float64) * qx[z].astype(np.float64)
        s64 = np.sign(e64).astype(np.int8)
        tie = np.where(py[z] != qy[z], np.where(py[z] > qy[z], 1, -1), np.where(qx[z] != px[z], np.where(qx[z] > px[z], 1, -1), 0))
        s[z] = np.where(s64 != 0, s64, tie).astype(np.int8)
    return e, s


def crosses(v32, f, o, d):
    """[F] bool: the kernel's predicate for every triangle of (v32 float32, f) and the ray from o (float32 [3]) along d."""
    kx, ky, kz, sx, sy, sz = _frame(d)
    x = v32 - o.astype(np.float32)[None]
    sxv = x[:, kx] - sx * x[:, kz]
    syv = x[:, ky] - sy * x[:, kz]
    # (a triangle whose sheared box does not hold the origin cannot count: skip it before the exact predicate -- exact, not a cull)
    fx, fy = sxv[f], syv[f]
    cand = np.nonzero((fx.min(1) <= 0) & (fx.max(1) >= 0) & (fy.min(1) <= 0) & (fy.max(1) >= 0))[0]
    out = np.zeros(len(f), bool)
    if len(cand) == 0:
        return out
    ff = f[cand]
    ax, ay, bx, by, cx, cy = sxv[ff[:, 0]], syv[ff[:, 0]], sxv[ff[:, 1]], syv[ff[:, 1]], sxv[ff[:, 2]], syv[ff[:, 2]]
    U, su = _edge_sign(bx, by, cx, cy)
    V, sv = _edge_sign(cx, cy, ax, ay)
    W, sw = _edge_sign(ax, ay, bx, by)
    ok = (su != 0) & (su == sv) & (su == sw)
    det = U + V + W
    ok &= det != 0
    z = sz * x[:, kz]
    T = U * z[ff[:, 0]] + V * z[ff[:, 1]] + W * z[ff[:, 2]]
    ok &= np.where(su > 0, T > 0, T < 0)
    out[cand] = ok
    return out


def crossings(v32, f, q32, rays):
    """[N, rays] int crossing counts of the recentred float32 mesh / queries, as nksr_mesh_occupancy counts them."""
    v32, q32, f = np.asarray(v32, np.float32), np.asarray(q32, np.float32), np.asarray(f, np.int64)
    out = np.zeros((len(q32), rays), np.int64)
    for i, o in enumerate(q32):
        for r in range(rays):
            out[i, r] = int(crosses(v32, f, o, DIRS[r]).sum())
    return out


def occupancy_from_counts(counts):
    return 2 * (counts & 1).sum(1) > counts.shape[1]


# ---- fp64 truth -----------------------------------------------------------------------------------------------------------------
def point_triangle_d2(p, a, b, c):
    """Squared distance of points p [N, 3] to triangles (a, b, c) [N, 3] (or broadcast), fp64: the minimum over the plane's foot
    point (when inside) and the three edges."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    safe = np.where(nn > 0, nn, 1.0)
    t = ((p - a) * n).sum(-1) / safe
    foot = p - t[..., None] * n
    inside = nn > 0
    for u, w in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(w - u, foot - u) * n).sum(-1) >= 0)
    best = np.where(inside, t * t * nn, np.inf)
    for u, w in ((a, b), (b, c), (c, a)):
        e = w - u
        ee = (e * e).sum(-1)
        s = np.clip(((p - u) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        r = p - (u + s[..., None] * e)
        best = np.minimum(best, (r * r).sum(-1))
    return best


def distance_bruteforce(v, f, q, upper=None, margin=0.0):
    """(distance [N], face [N]) of every query to the mesh in fp64; ties go to the smaller face.  With ``upper`` (a distance no
    smaller than the true one, minus ``margin``), faces whose fp64 box lies farther than upper + margin are skipped: exact all the
    same, since such a face cannot be the nearest."""
    v, q, f = np.asarray(v, np.float64), np.asarray(q, np.float64), np.asarray(f, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    dist, face = np.empty(len(q)), np.empty(len(q), np.int64)
    for i, p in enumerate(q):
        if upper is not None:
            g = np.maximum(np.maximum(lo - p, p - hi), 0.0)
            cand = np.nonzero((g * g).sum(1) <= (upper[i] + margin) ** 2)[0]
        else:
            cand = np.arange(len(f))
        d2 = point_triangle_d2(p[None], a[cand], b[cand], c[cand])
        k = int(np.argmin(d2))
        dist[i], face[i] = np.sqrt(d2[k]), cand[k]
    return dist, face


def distance_two_best(v, f, q):
    """(best, second best distance, argmin face) per query over every face, fp64."""
    v, q, f = np.asarray(v, np.float64), np.asarray(q, np.float64), np.asarray(f, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    two, face = np.empty((len(q), 2)), np.empty(len(q), np.int64)
    for i, p in enumerate(q):
        d2 = point_triangle_d2(p[None], a, b, c)
        k = np.argpartition(d2, 1)[:2] if len(d2) > 1 else np.array([0, 0])
        k = k[np.argsort(d2[k], kind='stable')]
        two[i], face[i] = np.sqrt(d2[k]), k[0]
    return two, face


def winding_number(v, f, q):
    """Generalised winding number (Jacobson et al. 2013) of every query, fp64 (Van Oosterom-Strackee solid angles / 4 pi)."""
    v, q, f = np.asarray(v, np.float64), np.asarray(q, np.float64), np.asarray(f, np.int64)
    out = np.empty(len(q))
    chunk = max(1, 1_000_000 // max(len(f), 1))
    for s in range(0, len(q), chunk):
        p = q[s:s + chunk, None, :]
        a, b, c = v[f[:, 0]][None] - p, v[f[:, 1]][None] - p, v[f[:, 2]][None] - p
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = 2.0 * np.arctan2(num, den).sum(1) / (4.0 * np.pi)
    return out


# ---- meshes with a known inside -----------------------------------------------------------------------------------------------------
_CUBE_FACES = [((-1, 0, 0), [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)]), ((1, 0, 0), [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)]),
               ((0, -1, 0), [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)]), ((0, 1, 0), [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)]),
               ((0, 0, -1), [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)]), ((0, 0, 1), [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])]


def voxel_mesh(vox, diag_seed=0):
    """Closed boundary of a union of unit voxels (integer corners), every square split into two triangles along a diagonal chosen
    at random, outward orientation.  (v float32 [V, 3], f int64 [F, 3])."""
    vox = {tuple(int(c) for c in x) for x in vox}
    rs = np.random.RandomState(diag_seed)
    idx, v, f = {}, [], []

    def vid(p):
        if p not in idx:
            idx[p] = len(v)
            v.append(p)
        return idx[p]
    for x in sorted(vox):
        for n, quad in _CUBE_FACES:
            if (x[0] + n[0], x[1] + n[1], x[2] + n[2]) in vox:
                continue
            q = [vid((x[0] + c[0], x[1] + c[1], x[2] + c[2])) for c in quad]
            if rs.randint(2):
                f += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                f += [[q[0], q[1], q[3]], [q[1], q[2], q[3]]]
    return np.array(v, np.float32), np.array(f, np.int64)


def voxel_union_is_manifold(vox):
    """No two voxels of the set meet only at an edge or a corner, and neither do two empty cells: in every 2 x 2 x 2 block the
    occupied cells are face-connected, and so are the empty ones.  Then the boundary is a closed 2-manifold."""
    vox = {tuple(int(c) for c in x) for x in vox}
    lo, hi = np.min(list(vox), 0) - 1, np.max(list(vox), 0) + 1
    cells = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    for x in range(lo[0], hi[0]):
        for y in range(lo[1], hi[1]):
            for z in range(lo[2], hi[2]):
                occ = {c: (x + c[0], y + c[1], z + c[2]) in vox for c in cells}
                for state in (True, False):
                    group = [c for c in cells if occ[c] == state]
                    if not group:
                        continue
                    seen, todo = {group[0]}, [group[0]]
                    while todo:
                        u = todo.pop()
                        for w in group:
                            if w not in seen and sum(abs(i - j) for i, j in zip(u, w)) == 1:
                                seen.add(w)
                                todo.append(w)
                    if len(seen) != len(group):
                        return False
    return True


def voxel_sets():
    """Named voxel unions: a block with a concave pocket, an L-shaped staircase, a hollow shell (a cavity inside: its boundary has
    two components), a random face-connected blob."""
    out = {}
    out['pocket'] = {(x, y, z) for x in range(4) for y in range(4) for z in range(3)} - {(1, 1, 2), (2, 1, 2), (1, 2, 2), (1, 1, 1)}
    out['stairs'] = {(x, y, z) for x in range(5) for y in range(3) for z in range(5 - x)}
    out['shell'] = {(x, y, z) for x in range(5) for y in range(5) for z in range(5)} - {(x, y, z) for x in range(1, 4) for y in range(1, 4)
                                                                                        for z in range(1, 3)}
    rs = np.random.RandomState(7)
    blob = {(0, 0, 0)}
    while len(blob) < 60:
        x = list(blob)[rs.randint(len(blob))]
        s = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)][rs.randint(6)]
        y = (x[0] + s[0], x[1] + s[1], x[2] + s[2])
        if max(abs(c) for c in y) <= 3 and voxel_union_is_manifold(blob | {y}):
            blob.add(y)
    out['blob'] = blob
    for k, s in out.items():
        assert voxel_union_is_manifold(s), k
    return out


def voxel_queries(vox, v, f):
    """Lattice points of step 0.5 over the padded box, minus those on the surface; (points float64 [N, 3], inside bool [N])."""
    vox = {tuple(x) for x in vox}
    lo, hi = np.min(list(vox), 0) - 1, np.max(list(vox), 0) + 2
    g = np.stack(np.meshgrid(*[np.arange(a, b + 0.25, 0.5) for a, b in zip(lo, hi)], indexing='ij'), -1).reshape(-1, 3)
    cell = np.floor(g).astype(np.int64)
    inside = np.array([tuple(c) in vox for c in cell])
    on = np.zeros(len(g), bool)
    d2 = np.full(len(g), np.inf)
    a, b, c = v[f[:, 0]].astype(np.float64), v[f[:, 1]].astype(np.float64), v[f[:, 2]].astype(np.float64)
    for s in range(0, len(f), 64):
        d2 = np.minimum(d2, point_triangle_d2(g[:, None], a[None, s:s + 64], b[None, s:s + 64], c[None, s:s + 64]).min(1))
    on = d2 < 1e-12
    return g[~on], inside[~on]


def convex_polyhedron(n_planes=40, seed=0, radius=1.0):
    """Triangulated hull of random points on a sphere: (v float32, f int64, planes (normal [P, 3], offset [P]) fp64 of the hull)."""
    from scipy.spatial import ConvexHull
    rs = np.random.RandomState(seed)
    p = rs.normal(size=(n_planes, 3))
    p = (radius * p / np.linalg.norm(p, axis=1, keepdims=True) * rs.uniform(0.7, 1.0, (n_planes, 1))).astype(np.float32)
    h = ConvexHull(p.astype(np.float64))
    f = h.simplices.astype(np.int64)
    v = p.astype(np.float64)
    flip = (np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]) * h.equations[:, :3]).sum(1) < 0
    f[flip] = f[flip][:, ::-1]                                                          # outward, as the winding number needs
    return p, f, h.equations[:, :3], h.equations[:, 3]


def inside_halfspaces(normals, offsets, q):
    """(inside, distance to the nearest plane) of q for a convex polyhedron given by its outward half-spaces n . x + d <= 0."""
    s = np.asarray(q, np.float64) @ normals.T + offsets[None]
    return (s < 0).all(1), np.abs(s).min(1)


def uv_sphere(nu=48, nv=24, r=0.4):
    th = np.linspace(0, np.pi, nv + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing='ij')
    v = np.concatenate([[[0, 0, r]], np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3),
                        [[0, 0, -r]]]).astype(np.float32)
    idx = lambda i, k: 1 + i * nu + k % nu                                              # noqa: E731
    f = []
    for k in range(nu):
        f.append([0, idx(0, k), idx(0, k + 1)])
        f.append([len(v) - 1, idx(nv - 2, k + 1), idx(nv - 2, k)])
    for i in range(nv - 2):
        for k in range(nu):
            f += [[idx(i, k), idx(i + 1, k), idx(i + 1, k + 1)], [idx(i, k), idx(i + 1, k + 1), idx(i, k + 1)]]
    return v, np.array(f, np.int64)


def torus(nu=64, nv=32, R=0.35, r=0.12):
    u = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    w = np.linspace(0, 2 * np.pi, nv, endpoint=False)
    U, W = np.meshgrid(u, w, indexing='ij')
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3).astype(np.float32)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int64)
