"""numpy restatement of nksr_amd/orient.py (csrc/orient.hip), an independent route to the same, unique result: Kruskal over the
sorted edge keys with a union-find that carries parity, where the kernels run Boruvka rounds.

Definition (include/nksr_hip.h).  Slot s = i k + c of the table idx [N, k] stands for the edge {i, idx[i, c]}; an entry < 0, >= N or
equal to i is ignored.  dot(a, b) = fl32(fl32(fl32(a0 b0) + fl32(a1 b1)) + fl32(a2 b2)) -- np.float32 arithmetic rounds every product
and sum to nearest and fuses nothing, so it gives the kernel's bits.  Weight w = max(fl32(1 - |dot|), 0), key (bits(w) << 32) | s,
flip bit of the edge dot < 0.  The minimum spanning forest over all slots is unique since the keys are distinct.  Sign of a component:
'+z': its point of largest z (lowest index on a tie; -0 counts as +0) ends with n_z >= 0; viewpoint v: with t = fl32(v - x), its point
of smallest dot(t, t) (lowest index on a tie) ends with dot(n, t) >= 0.  Components are numbered by their minimum point index."""
import numpy as np


def dot32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]           # float32 throughout, left to right


def edge_keys(normal, idx):
    """(key uint64 [E], u [E], v [E], flip bool [E]) of the valid slots"""
    normal = np.asarray(normal, np.float32)
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.reshape(-1)
    s = np.arange(n * k, dtype=np.uint64)
    ok = (j >= 0) & (j < n) & (j != rows)
    u, v, s = rows[ok], j[ok], s[ok]
    d = dot32(normal[u], normal[v])
    w = np.maximum(np.float32(1.0) - np.abs(d), np.float32(0.0)).astype(np.float32)
    key = (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | s
    return key, u, v, d < 0


def orient(xyz, normal, idx, viewpoint=None):
    """-> (flipped uint8 [N], component int32 [N], n_components)"""
    xyz, normal = np.asarray(xyz, np.float32), np.asarray(normal, np.float32)
    n = len(xyz)
    key, u, v, flip = edge_keys(normal, idx)
    order = np.argsort(key, kind='stable')
    parent = list(range(n))
    parity = [0] * n                    # sign of a node relative to its parent

    def find(x):
        """(root, parity of x relative to the root), with path compression"""
        path = []
        while parent[x] != x:
            path.append(x)
            x = parent[x]
        p = 0
        for y in reversed(path):        # from the root's child down to the start
            p ^= parity[y]
            parent[y], parity[y] = x, p
        return x, (parity[path[0]] if path else 0)

    for e in order.tolist():
        (ra, pa), (rb, pb) = find(int(u[e])), find(int(v[e]))
        if ra != rb:                    # an edge of the forest: sign(u) = sign(v) ^ flip
            parent[ra], parity[ra] = rb, pa ^ pb ^ int(flip[e])
    root = np.empty(n, np.int64)
    rel = np.empty(n, np.int64)
    for i in range(n):
        root[i], rel[i] = find(i)
    # dense labels by minimum point index
    _, first, inverse = np.unique(root, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first, kind='stable'), kind='stable')
    component = rank[inverse].astype(np.int32)
    ncomp = len(first)
    # seeds
    if viewpoint is None:
        score = xyz[:, 2] + np.float32(0.0)                              # (-0 + 0 = +0)
        seed_flip_of = normal[:, 2] < 0
    else:
        t = (np.asarray(viewpoint, np.float32)[None, :] - xyz).astype(np.float32)
        score = -dot32(t, t)
        seed_flip_of = dot32(normal, t) < 0
    flipped = np.zeros(n, np.uint8)
    for c in range(ncomp):
        members = np.nonzero(component == c)[0]
        s = members[np.argmax(score[members])]                           # argmax returns the first (lowest-index) maximum
        flipped[members] = (rel[members] ^ rel[s] ^ int(seed_flip_of[s])).astype(np.uint8)
    return flipped, component, ncomp


def apply(normal, flipped):
    normal = np.asarray(normal, np.float32)
    return np.where(flipped[:, None] != 0, -normal, normal)
