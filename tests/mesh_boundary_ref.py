"""numpy restatement of nksr_amd/mesh_boundary.py (csrc/meshbound.hip), written from DESIGN.md section 3.16 with plain loops and a
sequential walk: boundary half-edges, the umbrella walk, loops, measures (as lists of terms per loop in rank order; the sums are
math.fsum of them), selection and fill.  The edge table is that of tests/mesh_topology_ref.py.  Plus the small meshes the boundary
tests share (the others come from mesh_slice_ref / mesh_topology_ref)."""
import math

import numpy as np

import mesh_slice_ref as S
import mesh_topology_ref as T
from mesh_slice_ref import cube, cylinder, icosphere, strip  # noqa: F401
from mesh_topology_ref import random_soup, shuffled, three_fan, triangle_strip, two_cubes_sharing_a_vertex  # noqa: F401

BOUNDARY, INTERIOR = T.BOUNDARY, T.INTERIOR


def boundary_loops(v, f):
    """Everything ``MeshBoundary.loops`` returns, as a dict of numpy arrays (integers int32, -1 for none), plus per loop the lists of
    terms in rank order: ``length_terms``, ``area_terms`` [3 lists], ``moment_terms`` [3 lists] and ``p0``."""
    v = np.asarray(v).astype(np.float64)                # (fp32 widens exactly)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    nv, nf = len(v), len(f)
    t = T.edge_table(f, nv)
    cls, adj, ok = t['edge_classes'], t['face_adjacency'], t['face_valid']
    edge_of = {(int(a), int(b)): e for e, (a, b) in enumerate(t['edges'])}

    def ends(i, k):
        return int(f[i, k]), int(f[i, (k + 1) % 3])

    def cls_of(i, k):
        a, b = ends(i, k)
        return cls[edge_of[(min(a, b), max(a, b))]]

    # 1. boundary half-edges in ascending half-edge id
    halfedge = [3 * i + k for i in range(nf) if ok[i] for k in range(3) if cls_of(i, k) == BOUNDARY]
    bid = {h: b for b, h in enumerate(halfedge)}
    nb = len(halfedge)
    assert nb == t['boundary_edges']
    tail = [ends(h // 3, h % 3)[0] for h in halfedge]
    head = [ends(h // 3, h % 3)[1] for h in halfedge]

    # 2. rotation about the head (forward) and about the tail (backward)
    def walk(h, forward):
        i, k = divmod(h, 3)
        pivot = ends(i, k)[1 if forward else 0]
        steps = 0
        while True:
            k = (k + 1) % 3 if forward else (k + 2) % 3
            a, b = ends(i, k)
            assert (a if forward else b) == pivot
            c = cls_of(i, k)
            if c == BOUNDARY:
                return bid[3 * i + k], steps
            if c != INTERIOR:
                return -1, steps
            g = int(adj[i, k])
            twin = [q for q in range(3) if ends(g, q) == (b, a)]
            assert len(twin) == 1
            i, k = g, twin[0]
            steps += 1
            assert steps <= 3 * nf                      # (never: the orbit is a simple path)
    walks = [walk(h, True) for h in halfedge]
    succ = [w[0] for w in walks]
    pred = [-1] * nb
    for b, q in enumerate(succ):
        if q >= 0:
            assert pred[q] == -1 and tail[q] == head[b]                 # injective; head(b) is tail(succ)
            pred[q] = b
    assert pred == [walk(h, False)[0] for h in halfedge]

    # 3. loops: open chains from the elements without predecessor, cycles from their smallest id; ids ascend by representative
    rep, rank, chains = [-1] * nb, [-1] * nb, []
    for closed in (False, True):
        for s in range(nb):
            if rep[s] >= 0 or (not closed and pred[s] >= 0):
                continue
            chain, q = [], s
            while q >= 0 and rep[q] < 0:
                rep[q], rank[q] = s, len(chain)
                chain.append(q)
                q = succ[q]
            assert (q == s) if closed else (q == -1)
            chains.append((s, closed, chain))
    chains.sort(key=lambda c: c[0])
    loop_of = [-1] * nb
    loop_start, edge_start, loop_v, loop_he, simple = [0], [0], [], [], []
    length_terms, area_terms, moment_terms, p0s = [], [], [], []
    box = np.zeros((len(chains), 6))
    for l, (r, closed, chain) in enumerate(chains):
        p0 = v[tail[r]]
        lt, at, mt = [], ([], [], []), ([], [], [])
        for b in chain:
            loop_of[b] = l
            loop_v.append(tail[b])
            loop_he.append(halfedge[b])
            p, q = v[tail[b]], v[head[b]]
            d = q - p
            w = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            a, c = p - p0, q - p0
            lt.append(float(w))
            cross = (a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0])
            for k in range(3):
                at[k].append(float(0.5 * cross[k]) if closed else 0.0)
                mt[k].append(float(w * (0.5 * (a[k] + c[k]))))
        if not closed:
            loop_v.append(head[chain[-1]])
        pts = v[[tail[b] for b in chain] + [head[b] for b in chain]]
        box[l] = np.concatenate([pts.min(0), pts.max(0)])
        simple.append(len({tail[b] for b in chain}) == len(chain))
        loop_start.append(len(loop_v))
        edge_start.append(len(loop_he))
        length_terms.append(lt)
        area_terms.append(at)
        moment_terms.append(mt)
        p0s.append(p0)
    nl = len(chains)
    length = np.array([math.fsum(x) for x in length_terms], np.float64)
    area_vector = np.array([[math.fsum(x) for x in a] for a in area_terms], np.float64).reshape(-1, 3)
    centroid = np.zeros((nl, 3))
    for l in range(nl):
        m = np.array([math.fsum(x) for x in moment_terms[l]])
        centroid[l] = p0s[l] + m / length[l] if length[l] > 0 else p0s[l]
    i32 = lambda x: np.array(x, np.int32).reshape(-1)       # noqa: E731
    return {'n_boundary': nb, 'n_loops': nl, 'halfedge': i32(halfedge), 'tail': i32(tail), 'head': i32(head), 'face': i32([h // 3 for h in halfedge]),
            'succ': i32(succ), 'pred': i32(pred), 'boundary_loop': i32(loop_of), 'boundary_rank': i32(rank), 'loop_start': i32(loop_start),
            'loop_edge_start': i32(edge_start), 'loop_halfedges': i32(loop_he), 'loop_vertices': i32(loop_v), 'loop_rep': i32([c[0] for c in chains]),
            'loop_edges': i32([len(c[2]) for c in chains]), 'loop_closed': np.array([c[1] for c in chains], bool), 'loop_simple': np.array(simple, bool),
            'loop_length': length, 'loop_area_vector': area_vector, 'loop_area': np.sqrt((area_vector * area_vector).sum(1)),
            'loop_centroid': centroid, 'loop_box': box, 'length_terms': length_terms, 'area_terms': area_terms, 'moment_terms': moment_terms,
            'p0': np.array(p0s, np.float64).reshape(-1, 3), 'walk_steps': [w[1] for w in walks]}


INTEGER_ARRAYS = ('halfedge', 'tail', 'head', 'face', 'succ', 'pred', 'boundary_loop', 'boundary_rank', 'loop_start', 'loop_edge_start',
                  'loop_halfedges', 'loop_vertices', 'loop_rep', 'loop_edges', 'loop_closed', 'loop_simple')
FLOAT_ARRAYS = ('loop_length', 'loop_area_vector', 'loop_area', 'loop_centroid', 'loop_box')


def select(r, max_edges=None, max_length=None, max_area=None, simple_only=True):
    keep = r['loop_closed'].copy()
    if simple_only:
        keep &= r['loop_simple']
    if max_edges is not None:
        keep &= r['loop_edges'] <= max_edges
    if max_length is not None:
        keep &= r['loop_length'] <= max_length
    if max_area is not None:
        keep &= r['loop_area'] <= max_area
    return keep


def fill(v, f, r, keep, method='centroid', colors=None):
    """(v2, f2, c2, new_vertex_mask, new_face_loop, colour_terms): plain loops over the kept loops in ascending id; ``colour_terms`` =
    per new vertex and channel the list of the loop's vertex colours in rank order (their fsum / m is the mean)."""
    v, f = np.asarray(v), np.asarray(f).reshape(-1, 3)
    keep = np.asarray(keep, bool)
    if (keep & ~r['loop_closed']).any():
        raise ValueError('open chains cannot be closed')
    if method == 'fan' and (keep & ~r['loop_simple']).any():
        raise ValueError('fan needs simple loops')
    nv = len(v)
    new_v, new_f, face_loop, colour_terms = [], [], [], []
    for l in np.nonzero(keep)[0]:
        ids = r['loop_vertices'][r['loop_start'][l]:r['loop_start'][l + 1]]
        m = len(ids)
        if method == 'centroid':
            apex = nv + len(new_v)
            new_v.append(r['loop_centroid'][l].astype(v.dtype))
            for i in range(m):
                new_f.append([ids[(i + 1) % m], ids[i], apex])
                face_loop.append(l)
            if colors is not None:
                colour_terms.append([[float(colors[j, ch]) for j in ids] for ch in range(colors.shape[1])])
        else:
            for i in range(1, m - 1):
                new_f.append([ids[i + 1], ids[i], ids[0]])
                face_loop.append(l)
    v2 = np.concatenate([v, np.array(new_v, v.dtype).reshape(-1, 3)])
    f2 = np.concatenate([f, np.array(new_f, f.dtype).reshape(-1, 3)])
    mask = np.arange(len(v2)) >= nv
    c2 = None
    if colors is not None:
        means = np.array([[math.fsum(t) / len(t) for t in per] for per in colour_terms], np.float64).reshape(-1, colors.shape[1])
        c2 = np.concatenate([colors, means.astype(colors.dtype)])
    return v2, f2, c2, mask, np.array(face_loop, np.int32), colour_terms


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def triangle():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int64)


def open_tetrahedron():
    """The dyadic tetrahedron less its last face: one loop of 3."""
    v, f = S.tetrahedron()
    return v, f[:-1]


def open_cube():
    """The unit cube less its top side: one loop of 4, length 4, area 1."""
    v, f = S.cube()
    return v, np.delete(f, [2, 3], 0)


def strip_less_two_quads(nx=4, ny=4):
    """strip(nx, ny) without the quads (1, 1) and (2, 2), which touch in the vertex (2, 2): two loops of 4 through it, and the rim."""
    v, f = S.strip(nx, ny)
    gone = [2 * (a * ny + b) + k for a, b in ((1, 1), (2, 2)) for k in (0, 1)]
    return v, np.delete(f, gone, 0), 2 * (ny + 1) + 2


def two_cubes_opened_at_the_shared_vertex():
    """Two cubes welded in one corner, each less one face at that corner: two loops of 3 that touch there.  (v, f, the vertex)"""
    v, f = T.two_cubes_sharing_a_vertex()
    shared = int(np.nonzero((v == 1).all(1))[0][0])
    at = np.nonzero((f == shared).any(1))[0]
    assert len(f) == 24                                                             # (12 faces per cube, the first cube's first)
    return v, np.delete(f, [at[at < 12][0], at[at >= 12][0]], 0), shared


def disc_fan(n=1000):
    """n triangles (0, r_i, r_i+1) about the centre 0 over n + 1 rim vertices: one wedge of the disc is missing, and the successor of
    the half-edge that runs into the centre is found after n - 1 crossings."""
    a = 2.0 * np.pi * np.arange(n + 1) / (n + 1)
    v = np.concatenate([np.zeros((1, 3)), np.stack([np.cos(a), np.sin(a), np.zeros(n + 1)], 1)])
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), i + 1, i + 2], 1)


def pinched_disc(n=4):
    """strip(n, 1) with its last corner welded to its first: a disc whose border passes that vertex twice.  (Vertex 2 n + 1 stays,
    unreferenced.)"""
    v, f = S.strip(n, 1)
    f = f.copy()
    f[f == 2 * n + 1] = 0
    return v, f


def holed_icosphere(subdivisions=3, n_holes=12, seed=3):
    """The icosphere less the stars of ``n_holes`` vertices no two of which are nearer than three edges (vertex 0, of valence 5, among
    them), shuffled: that many separate holes of 5 or 6 edges.  (v, f)"""
    v, f = S.icosphere(subdivisions)
    nbr = [set() for _ in range(len(v))]
    for a, b, c in f:
        nbr[a] |= {b, c}
        nbr[b] |= {a, c}
        nbr[c] |= {a, b}
    picked, blocked = [], set()
    for i in [0] + list(np.random.RandomState(seed).permutation(len(v))):
        if len(picked) < n_holes and i not in blocked:
            picked.append(int(i))
            ring2 = set().union(*[nbr[j] for j in nbr[i]]) | nbr[i] | {int(i)}
            blocked |= set().union(*[nbr[j] for j in ring2]) | ring2
    assert len(picked) == n_holes
    f = f[~np.isin(f, picked).any(1)]
    return T.shuffled(v, f, seed)
