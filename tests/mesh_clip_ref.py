"""numpy restatement of nksr_amd/mesh_clip.py (csrc/meshclip.hip), written from the definitions of DESIGN.md section 3.17 with plain loops:
every face's walk is built element by element, its pieces are read off the walk and fanned.  Like tests/mesh_slice_ref.py it takes the
heights as an argument -- in the GPU tests the heights the GPU reports, so that every side decision is made from the same numbers --
and optionally the points (else it computes its own, operation by operation as the slicer states them).  The edge table is that of
tests/mesh_topology_ref.py; the meshes are those of tests/mesh_slice_ref.py."""
import math
from bisect import bisect_right

import numpy as np

import mesh_topology_ref as T
from mesh_slice_ref import cube, cylinder, heights, icosphere, merged, strip, tetrahedron, torus, unit, uv_sphere  # noqa: F401


def split_mesh(v, f, normal, offsets, h, points=None, attr=None):
    """Everything ``MeshClipper.split`` returns, as a dict of numpy arrays.  ``normal`` is unused but for symmetry with ``slice_mesh``
    (the heights carry it)."""
    v = np.asarray(v).astype(np.float64)                # (fp32 widens exactly)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    o = [float(x) for x in np.asarray(offsets, np.float64).reshape(-1)]
    assert all(math.isfinite(x) for x in o) and all(b > a for a, b in zip(o, o[1:]))
    h = [float(x) for x in np.asarray(h, np.float64)]
    nv, nf = len(v), len(f)
    t = T.edge_table(f, nv)
    edges, ok = t['edges'], t['face_valid']
    edge_of = {(int(a), int(b)): e for e, (a, b) in enumerate(edges)}
    slab = [bisect_right(o, x) for x in h]              # the planes at or below the vertex: it is ABOVE those

    # cut points: the slicer's, one per (edge, plane in (min, max]), id = point_start[e] + (j - lo_e)
    lo_e, point_start, pts, p_edge, p_plane, p_attr = [], [0], [], [], [], []
    a64 = None if attr is None else np.asarray(attr).astype(np.float64)
    for e, (a, b) in enumerate(edges):
        lo, hi = min(slab[a], slab[b]), max(slab[a], slab[b])
        lo_e.append(lo)
        for j in range(lo, hi):
            assert min(h[a], h[b]) < o[j] <= max(h[a], h[b])
            tt = np.float64(o[j] - h[a]) / np.float64(h[b] - h[a])
            pts.append(v[a] + tt * (v[b] - v[a]))
            if a64 is not None:
                p_attr.append(a64[a] + tt * (a64[b] - a64[a]))
            p_edge.append(e)
            p_plane.append(j)
        point_start.append(len(pts))
    own = np.array(pts, np.float64).reshape(-1, 3)
    pm = own if points is None else np.asarray(points, np.float64).reshape(-1, 3)
    assert pm.shape == own.shape

    # pieces: walk c0 -> c1 -> c2 -> c0; a corner belongs to the piece of its slab, a point of plane j to pieces j and j + 1
    f2, source, part, face_start = [], [], [], [0]
    for i in range(nf):
        if ok[i]:
            c = [int(x) for x in f[i]]
            pieces = {}
            for k in range(3):
                a, b = c[k], c[(k + 1) % 3]
                sa, sb = slab[a], slab[b]
                pieces.setdefault(sa, []).append(a)
                e = edge_of[(min(a, b), max(a, b))]
                for j in (range(sa, sb) if sa < sb else range(sa - 1, sb - 1, -1)):      # the planes in travel order
                    assert lo_e[e] <= j < lo_e[e] + (point_start[e + 1] - point_start[e])
                    p = nv + point_start[e] + (j - lo_e[e])
                    pieces.setdefault(j, []).append(p)
                    pieces.setdefault(j + 1, []).append(p)
            smin, smax = min(slab[x] for x in c), max(slab[x] for x in c)
            assert sorted(pieces) == list(range(smin, smax + 1))
            for s in range(smin, smax + 1):
                m = pieces[s]
                assert 3 <= len(m) <= 5 and len(set(m)) == len(m)
                for q in range(1, len(m) - 1):
                    f2.append((m[0], m[q], m[q + 1]))
                    source.append(i)
                    part.append(s)
            assert len(f2) - face_start[-1] == 2 * (smax - smin) + 1
        face_start.append(len(f2))
    i32 = lambda x, shape=(-1,): np.array(x, np.int32).reshape(shape)       # noqa: E731
    f2 = i32(f2, (-1, 3))
    v2 = np.concatenate([v, pm])
    bits = v2.view(np.int64)[f2]                        # [F2, 3, 3]
    same = np.zeros(len(f2), bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        same |= (bits[:, a] == bits[:, b]).all(1) | (f2[:, a] == f2[:, b])
    return {'v2_64': v2, 'points64': own, 'f2': f2, 'face_source': i32(source), 'face_part': i32(part),
            'face_start': np.array(face_start, np.int64), 'point_edge': i32(p_edge), 'point_plane': i32(p_plane),
            'point_start': np.array(point_start, np.int64),
            'attr2_64': None if a64 is None else np.concatenate([a64, np.array(p_attr, np.float64).reshape(-1, a64.shape[1])]),
            'n_points': len(pts), 'n_faces': len(f2), 'n_parts': len(o) + 1, 'n_dropped': int(nf - np.count_nonzero(ok)),
            'n_degenerate': int(same.sum()), 'slab': i32(slab)}


INTEGER_ARRAYS = ('f2', 'face_source', 'face_part', 'face_start', 'point_edge', 'point_plane', 'point_start')
GROUP_ARRAYS = ('f', 'face_order', 'vertex_source', 'part_vertex_start', 'part_face_start', 'labels')


def group(f, labels, n_labels):
    """The exploded mesh: one new vertex per distinct (label, vertex), numbered label-major and then by old vertex id; the faces stably
    sorted by label."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    labels = np.asarray(labels, np.int64).reshape(-1)
    assert len(labels) == len(f) and (len(f) == 0 or (labels.min() >= 0 and labels.max() < n_labels))
    keys = sorted({(int(labels[i]), int(x)) for i in range(len(f)) for x in f[i]})
    new = {k: r for r, k in enumerate(keys)}
    order = sorted(range(len(f)), key=lambda i: labels[i])          # (sorted is stable)
    f_out = [[new[(int(labels[i]), int(x))] for x in f[i]] for i in order]
    vstart = [sum(1 for k in keys if k[0] < j) for j in range(n_labels + 1)]
    fstart = [int(np.count_nonzero(labels < j)) for j in range(n_labels + 1)]
    return {'f': np.array(f_out, np.int32).reshape(-1, 3), 'face_order': np.array(order, np.int32), 'labels': labels[order].astype(np.int32),
            'vertex_source': np.array([k[1] for k in keys], np.int32), 'part_vertex_start': np.array(vstart, np.int64),
            'part_face_start': np.array(fstart, np.int64)}


def part_mesh(g, j, v, c=None):
    """(v, f, c) of part j of ``group``'s result over the vertices ``v``: local indices."""
    a, b = g['part_vertex_start'][j:j + 2]
    fa, fb = g['part_face_start'][j:j + 2]
    src = g['vertex_source'][a:b]
    return v[src], (g['f'][fa:fb] - a).astype(np.int32), None if c is None else c[src]


def compact(v, f, keep, c=None):
    """The kept faces in their order, the vertices they name in theirs (``mesh_topology.compact_mesh`` on valid faces)."""
    f = np.asarray(f, np.int64).reshape(-1, 3)[np.asarray(keep, bool)]
    used = np.unique(f)
    remap = np.full(len(v), -1, np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f].astype(np.int32), None if c is None else c[used]


def axis_normal(axis):
    n = np.zeros(3)
    n[axis] = 1.0
    return n


def clip_box(v, f, lo, hi, attr=None):
    """``MeshClipper.clip_box``: x, y, z in turn, the middle part of two planes, every stage in the dtype of ``v``.  Along an axis the
    height is the coordinate itself (n = e_axis: the fused sum adds exact zeros), so the restatement needs no reported heights."""
    v, f = np.asarray(v), np.asarray(f, np.int64).reshape(-1, 3)
    for axis in range(3):
        r = split_mesh(v, f, axis_normal(axis), [lo[axis], hi[axis]], v[:, axis].astype(np.float64), attr=attr)
        c2 = None if attr is None else r['attr2_64'].astype(np.asarray(attr).dtype)
        v, f, attr = compact(r['v2_64'].astype(v.dtype), r['f2'], r['face_part'] == 1, c2)
    return v, f, attr


def interval_levels(x, step, origin=0.0):
    """origin + k step in (min, max] of the coordinates ``x`` (those of the referenced vertices)."""
    if len(x) == 0:
        return np.zeros(0)
    lo, hi = float(np.min(x)), float(np.max(x))
    k0, k1 = math.floor((lo - origin) / step) - 1, math.floor((hi - origin) / step) + 1
    lv = np.arange(k0, k1 + 1, dtype=np.float64) * step
    if origin != 0.0:
        lv = origin + lv
    return lv[(lv > lo) & (lv <= hi)]


def tiles(v, f, levels, axes, attr=None):
    """``MeshClipper.tiles`` at the given levels (two arrays): (group result, v64 of the second split, attr of it, (nx, ny))."""
    v, f = np.asarray(v), np.asarray(f, np.int64).reshape(-1, 3)
    a = split_mesh(v, f, axis_normal(axes[0]), levels[0], v[:, axes[0]].astype(np.float64), attr=attr)
    v1 = a['v2_64'].astype(v.dtype)
    c1 = None if attr is None else a['attr2_64'].astype(np.asarray(attr).dtype)
    b = split_mesh(v1, a['f2'], axis_normal(axes[1]), levels[1], v1[:, axes[1]].astype(np.float64), attr=c1)
    nx, ny = len(levels[0]) + 1, len(levels[1]) + 1
    labels = a['face_part'][b['face_source']].astype(np.int64) * ny + b['face_part']
    c2 = None if attr is None else b['attr2_64'].astype(np.asarray(attr).dtype)
    return group(b['f2'], labels, nx * ny), b['v2_64'], c2, (nx, ny)


def face_areas(v, f):
    """Areas and (unnormalised) normals of the faces, fp64."""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((n * n).sum(1)), n


EPS = np.finfo(np.float64).eps


def area_bound(v, f, r):
    """Per input face, a bound on |sum of its triangles' areas - its area|, both evaluated in fp64.

    A cut point is a + t (b - a) with t and the three operations rounded: per coordinate it lies within 4 eps (|a| + |b|) <= 8 eps M of
    the exact point of the edge (the slicer's point bound), M the largest |coordinate| of the face, so within
    d = 8 sqrt(3) eps M in space.  With exact points the pieces tile the face and the areas add up exactly.  Moving the corners of a
    triangle (p, q, r) by at most d each changes (q - p) x (r - p) by at most 2 d (|q - p| + |r - p|) + 4 d^2, its area by half of that;
    every edge of every output triangle is at most D, the face's longest edge, so a triangle's area moves by at most 2 d D + 2 d^2.
    Evaluating an area in fp64 (differences, a cross product, a square root) costs at most 8 eps D^2 more.  With n = 2 k + 1 triangles
    and the face itself:  bound_f = (n + 1) (2 d D + 2 d^2 + 8 eps D^2).
    The bound is relative to D (D + M) -- lengths, never the area: a sliver has no relative bound -- and it carries M beside the
    |b - a| |c - a| <= D^2 one might hope for, because the rounding of a point scales with the size of the coordinates, not of the edge.
    (Well-conditioned triangles near the origin measure about 4e-15 relative: a sanity check, not the bound.)"""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    out = np.zeros(len(f))
    n_tri = np.diff(r['face_start'])
    for i in np.nonzero(n_tri)[0]:
        p = v[f[i]]
        big = max(np.linalg.norm(p[0] - p[1]), np.linalg.norm(p[1] - p[2]), np.linalg.norm(p[2] - p[0]))
        d = 8.0 * np.sqrt(3.0) * EPS * np.abs(p).max()
        out[i] = (n_tri[i] + 1) * (2 * d * big + 2 * d * d + 8 * EPS * big * big)
    return out
