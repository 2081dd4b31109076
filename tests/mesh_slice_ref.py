"""numpy restatement of nksr_amd/mesh_slice.py (csrc/meshslice.hip), written from items 2-7 of DESIGN.md section 3.15 with plain loops
and a sequential chain walk.  It takes the heights as an argument -- in the GPU tests the heights the GPU reports, so that every side
decision is made from the same numbers (the heights themselves are checked against numpy separately) -- and, for the measures alone,
optionally the points to measure (the GPU tests pass the reported points, which they have compared with the restatement's own first:
a length is a function of its end points, and two point sets that agree to rounding can give short segments whose lengths do not).
The edge table is that of tests/mesh_topology_ref.py.  Plus the small meshes the slicing tests share."""
import math
from bisect import bisect_right

import numpy as np

import mesh_topology_ref as T
from mesh_topology_ref import torus, uv_sphere  # noqa: F401

INTERIOR = T.INTERIOR


def unit(normal):
    n = np.asarray(normal, np.float64).reshape(3)
    n = n / np.max(np.abs(n))
    return n / math.sqrt(float(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]))


def heights(v, normal):
    """h = n . x in fp64, products and sums rounded one by one (the GPU fuses them: equal to within 3 eps sum |n_i x_i|)."""
    v, n = np.asarray(v).astype(np.float64), unit(normal)
    return n[0] * v[:, 0] + n[1] * v[:, 1] + n[2] * v[:, 2]


def slice_mesh(v, f, normal, offsets, h, points=None):
    """Everything ``MeshSlicer.slice`` returns, as a dict of numpy arrays (integers int32, -1 for none) plus the lists of terms
    ``length_terms`` / ``area_terms`` per polyline in rank order; lengths and areas are their math.fsum."""
    v = np.asarray(v).astype(np.float64)                # (fp32 widens exactly)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    n = np.asarray(normal, np.float64).reshape(3)       # the UNIT normal, taken as it is (``unit`` makes one)
    o = [float(x) for x in np.asarray(offsets, np.float64).reshape(-1)]
    assert all(math.isfinite(x) for x in o) and all(b > a for a, b in zip(o, o[1:]))
    h = [float(x) for x in np.asarray(h, np.float64)]
    nv, nf, npl = len(v), len(f), len(o)
    t = T.edge_table(f, nv)
    edges, cls, adj, ok = t['edges'], t['edge_classes'], t['face_adjacency'], t['face_valid']
    edge_of = {(int(a), int(b)): e for e, (a, b) in enumerate(edges)}

    # 3. points: one per (edge, plane in (min, max]), id = point_start[e] + (j - lo_e)
    lo_e, point_start, pts, p_edge, p_plane = [], [0], [], [], []
    for e, (a, b) in enumerate(edges):
        ha, hb = h[a], h[b]
        lo, hi = bisect_right(o, min(ha, hb)), bisect_right(o, max(ha, hb))
        lo_e.append(lo)
        for j in range(lo, hi):
            assert min(ha, hb) < o[j] <= max(ha, hb)
            tt = np.float64(o[j] - ha) / np.float64(hb - ha)
            pts.append(v[a] + tt * (v[b] - v[a]))
            p_edge.append(e)
            p_plane.append(j)
        point_start.append(len(pts))
    own_points = np.array(pts, np.float64).reshape(-1, 3)

    # 2. + 4. segments: one per (face, crossed plane), face-major, plane ascending
    lo_f, seg_start = np.zeros(nf, np.int64), np.zeros(nf + 1, np.int64)
    seg, s_face, s_plane, up_half = [], [], [], []
    for i in range(nf):
        if ok[i]:
            hc = [h[c] for c in f[i]]
            lo, hi = bisect_right(o, min(hc)), bisect_right(o, max(hc))
            lo_f[i] = lo
            for j in range(lo, hi):
                above = [x >= o[j] for x in hc]
                assert min(hc) < o[j] <= max(hc) and not all(above) and any(above)
                down = [k for k in range(3) if above[k] and not above[(k + 1) % 3]]
                up = [k for k in range(3) if not above[k] and above[(k + 1) % 3]]
                assert len(down) == 1 and len(up) == 1              # exactly one half-edge goes down and one goes up
                ends = []
                for k in (down[0], up[0]):
                    a, b = int(f[i, k]), int(f[i, (k + 1) % 3])
                    e = edge_of[(min(a, b), max(a, b))]
                    assert lo_e[e] <= j < lo_e[e] + (point_start[e + 1] - point_start[e])
                    ends.append(point_start[e] + (j - lo_e[e]))
                seg.append(ends)
                s_face.append(i)
                s_plane.append(j)
                up_half.append((up[0], down[0]))
        seg_start[i + 1] = len(seg)
    ns = len(seg)

    # 5. successor: the segment of the face across the half-edge that carries the head, same plane, INTERIOR edges only
    def across(s, k):
        i, j = s_face[s], s_plane[s]
        a, b = int(f[i, k]), int(f[i, (k + 1) % 3])
        if cls[edge_of[(min(a, b), max(a, b))]] != INTERIOR:
            return -1
        g = int(adj[i, k])
        assert g >= 0 and lo_f[g] <= j < lo_f[g] + (seg_start[g + 1] - seg_start[g])
        return int(seg_start[g] + (j - lo_f[g]))
    succ = [across(s, up_half[s][0]) for s in range(ns)]
    pred = [-1] * ns
    for s, q in enumerate(succ):
        if q >= 0:
            assert pred[q] == -1 and seg[q][0] == seg[s][1] and s_plane[q] == s_plane[s]       # injective; head(s) is tail(succ)
            pred[q] = s
    assert pred == [across(s, up_half[s][1]) for s in range(ns)]

    # 6. polylines: sequential walks; open chains from the segments without predecessor, then cycles from their smallest id
    rep, rank, chains = [-1] * ns, [-1] * ns, []
    for closed in (False, True):
        for s in range(ns):
            if rep[s] >= 0 or (not closed and pred[s] >= 0):
                continue
            chain, q = [], s
            while q >= 0 and rep[q] < 0:
                rep[q], rank[q] = s, len(chain)
                chain.append(q)
                q = succ[q]
            assert (q == s) if closed else (q == -1)
            chains.append((s_plane[s], s, closed, chain))
    chains.sort(key=lambda c: (c[0], c[1]))
    pm = own_points if points is None else np.asarray(points, np.float64).reshape(-1, 3)
    poly_start, poly_points, seg_poly = [0], [], [-1] * ns
    length_terms, area_terms = [], []
    for l, (_, r, closed, chain) in enumerate(chains):
        p0 = pm[seg[r][0]] if ns else None
        lt, at = [], []
        for s in chain:
            seg_poly[s] = l
            poly_points.append(seg[s][0])
            p, q = pm[seg[s][0]], pm[seg[s][1]]
            d = q - p
            lt.append(float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])))
            if closed:
                a, b = p - p0, q - p0
                c = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
                at.append(float(0.5 * (n[0] * c[0] + n[1] * c[1] + n[2] * c[2])))
            else:
                at.append(0.0)
        if not closed:
            poly_points.append(seg[chain[-1]][1])
        poly_start.append(len(poly_points))
        length_terms.append(lt)
        area_terms.append(at)
    nl = len(chains)
    poly_plane = np.array([c[0] for c in chains], np.int32)
    poly_closed = np.array([c[2] for c in chains], bool)
    poly_length = np.array([math.fsum(x) for x in length_terms], np.float64)
    poly_area = np.array([math.fsum(x) for x in area_terms], np.float64)
    plane_poly_start = np.searchsorted(poly_plane, np.arange(npl + 1)).astype(np.int32)
    of = [range(plane_poly_start[j], plane_poly_start[j + 1]) for j in range(npl)]
    i32 = lambda x, shape=(-1,): np.array(x, np.int32).reshape(shape)       # noqa: E731
    return {'points64': own_points, 'point_edge': i32(p_edge), 'point_plane': i32(p_plane), 'point_start': np.array(point_start, np.int64),
            'segments': i32(seg, (-1, 2)), 'segment_face': i32(s_face), 'segment_plane': i32(s_plane), 'seg_start': seg_start,
            'succ': i32(succ), 'pred': i32(pred), 'segment_polyline': i32(seg_poly), 'segment_rank': i32(rank),
            'polyline_start': i32(poly_start), 'polyline_points': i32(poly_points), 'polyline_rep': i32([c[1] for c in chains]),
            'polyline_closed': poly_closed, 'polyline_plane': poly_plane, 'polyline_length': poly_length, 'polyline_area': poly_area,
            'plane_length': np.array([math.fsum(poly_length[k] for k in r) for r in of], np.float64),
            'plane_area': np.array([math.fsum(poly_area[k] for k in r) for r in of], np.float64),
            'plane_open': i32([sum(1 for k in r if not poly_closed[k]) for r in of]), 'plane_polyline_start': plane_poly_start,
            'length_terms': length_terms, 'area_terms': area_terms, 'n_points': len(pts), 'n_segments': ns, 'n_polylines': nl}


INTEGER_ARRAYS = ('point_edge', 'point_plane', 'point_start', 'segments', 'segment_face', 'segment_plane', 'seg_start', 'succ', 'pred',
                  'segment_polyline', 'segment_rank', 'polyline_start', 'polyline_points', 'polyline_rep', 'polyline_closed', 'polyline_plane',
                  'plane_open', 'plane_polyline_start')


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    """Dyadic corners, outward faces; heights along z: 0, 0, 0, 1 -- along (1, 1, 1): 0, 1, 1, 1."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)


def cube(lo=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0)):
    """The axis-aligned box as 12 outward triangles."""
    c = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float64)
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]],
                 np.int64)
    return (np.asarray(lo, np.float64) + c * np.asarray(size, np.float64)).astype(np.float32), f


def strip(nx, ny):
    """An open nx x ny grid of unit squares in the plane z = x / 4 (two triangles each, normals up): its sections along x are open."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing='ij')
    v = np.stack([i, j, i / 4.0], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda a, b: a * (ny + 1) + b         # noqa: E731
    f = []
    for a in range(nx):
        for b in range(ny):
            f += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    return v, np.array(f, np.int64)


def cylinder(n_round, rows=2, radius=1.0, roll=None):
    """An open tube round z: n_round quads per row, outward normals, heights z = 0 .. rows; the face order rolled by ``roll`` (default: half
    the faces), so that the smallest segment id of a loop lies in the middle of it."""
    a = 2.0 * np.pi * np.arange(n_round) / n_round
    v = np.concatenate([np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n_round, float(r))], 1) for r in range(rows + 1)])
    f = []
    for r in range(rows):
        for i in range(n_round):
            p, q = r * n_round + i, r * n_round + (i + 1) % n_round
            f += [[p, q, q + n_round], [p, q + n_round, p + n_round]]
    f = np.array(f, np.int64)
    return v.astype(np.float64), np.roll(f, len(f) // 2 + 1 if roll is None else roll, axis=0)


def icosphere(subdivisions, radius=1.0):
    """20 * 4^subdivisions outward triangles on the sphere of ``radius``."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float64) * radius, np.array(f, np.int64)


def merged(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float64))
        fs.append(np.asarray(f, np.int64) + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(fs)
