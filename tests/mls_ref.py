"""numpy / scipy restatement of moving-least-squares projection, written from the definition (csrc/mls.hip's header comment) in float64,
and the test clouds of tests/test_mls_cpu.py and tests/test_gpu_mls.py.

Neighbours of a query q: the points p of the float32 cloud with |p - q|^2 <= fl32(h)^2 (inclusive, float64 arithmetic on the float32
coordinates: what the kernel's fp32 predicate decides wherever no point lies within rounding of the radius -- ``radius_gap`` measures
that -- and exactly on a lattice cloud, where both are exact).  Weights w = exp(-|d|^2 / sigma^2), d = p - q.  Plane: W = sum w,
m = sum w d / W, C = sum w (d - m)(d - m)^T, eigenvalues l0 <= l1 <= l2 (``numpy.linalg.eigh``), n the eigenvector of l0, o = (m . n) n.
Order 1: x' = q + o.  Order 2: r = d - o, x = r . u / h, y = r . v / h, z = r . n / h, z ~ a0 + a1 x + a2 y + a3 x^2 + a4 x y + a5 y^2 by the
weighted normal equations and Cholesky; x' = q + o + a0 h n; normal (n - a1 u - a2 v) / |.|; curvatures from the fit's derivatives.
Sign of n: with normals, flipped when sum w (n_i . n) < 0; without, the component with the largest magnitude is positive (the lowest axis on a
tie).  order_used = 0: fewer than min_neighbors neighbours, W not positive, or l1 <= max(1e-12 l2, 1e-14 W h^2); order 2 falls back to 1 when a Cholesky pivot
is <= 1e-12 x the largest diagonal entry.  Everything is batched over the queries: neighbour lists padded to the longest, masked by w = 0.
"""
import functools

import numpy as np
from scipy.spatial import cKDTree

RANK_TOL = 1e-12
ROUNDING_FLOOR = 1e-14             # x W h^2: an eigenvalue below it is the rounding of the kernel's shifted sums
MIN_NEIGHBORS = {1: (3, 3), 2: (6, 8)}


def neighbours(xyz, query, h):
    """(idx int64 [Q, K] padded with 0, mask bool [Q, K], d float64 [Q, K, 3] = p - q) for h already rounded to float32"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    q = np.asarray(query, np.float32).astype(np.float64)
    lists = cKDTree(x).query_ball_point(q, h * (1.0 + 1e-6), return_sorted=True) if len(q) else []
    K = max([len(l) for l in lists] + [1])
    idx = np.zeros((len(q), K), np.int64)
    mask = np.zeros((len(q), K), bool)
    for i, l in enumerate(lists):
        idx[i, :len(l)] = l
        mask[i, :len(l)] = True
    d = x[idx] - q[:, None, :]
    mask &= (d * d).sum(2) <= h * h
    return idx, mask, d


def radius_gap(xyz, query, radius):
    """the smallest | |p - q| / h - 1 | over all pairs: how far the nearest pair is from sitting AT the radius"""
    h = float(np.float32(radius))
    x = np.asarray(xyz, np.float32).astype(np.float64)
    q = np.asarray(query, np.float32).astype(np.float64)
    tree = cKDTree(x)
    gap = np.inf
    for i, l in enumerate(tree.query_ball_point(q, h * 1.001)):
        r = np.sqrt(((x[l] - q[i]) ** 2).sum(1)) / h
        r = r[r > 0.999]
        if len(r):
            gap = min(gap, float(np.abs(r - 1.0).min()))
    return gap


def cholesky_solve(A, b):
    """Batched Cholesky solve of A [Q, 6, 6] a = b [Q, 6] -> (a, ok bool [Q], ratio [Q] = the smallest pivot / the largest diagonal
    entry).  A pivot <= RANK_TOL x the largest diagonal entry: ok False (that row's solution is meaningless)."""
    n = A.shape[1]
    L = np.zeros_like(A)
    dmax = np.max(np.diagonal(A, axis1=1, axis2=2), axis=1)
    ok = np.ones(len(A), bool)
    ratio = np.full(len(A), np.inf)
    safe = np.where(dmax > 0, dmax, 1.0)
    for j in range(n):
        s = A[:, j, j] - (L[:, j, :j] ** 2).sum(1)
        ratio = np.minimum(ratio, s / safe)
        bad = ~(s > RANK_TOL * dmax)
        ok &= ~bad
        s = np.where(bad, 1.0, s)
        L[:, j, j] = np.sqrt(s)
        for r in range(j + 1, n):
            L[:, r, j] = (A[:, r, j] - (L[:, r, :j] * L[:, j, :j]).sum(1)) / L[:, j, j]
    y = np.zeros_like(b)
    for r in range(n):
        y[:, r] = (b[:, r] - (L[:, r, :r] * y[:, :r]).sum(1)) / L[:, r, r]
    a = np.zeros_like(b)
    for r in range(n - 1, -1, -1):
        a[:, r] = (y[:, r] - (L[:, r + 1:, r] * a[:, r + 1:]).sum(1)) / L[:, r, r]
    return a, ok, ratio


def mls_project(xyz, radius, normal=None, query=None, order=2, sigma=None, min_neighbors=None, rotate_frame=0.0):
    """-> dict(position [Q, 3], normal [Q, 3], mean_curvature, gaussian_curvature, variation [Q], count int32 [Q], order_used int8 [Q],
    and the diagnostics cond [Q] (2-norm condition number of the 6 x 6 system), pivot_ratio [Q], eig_ratio [Q] = l0 / l1,
    sign_margin [Q] = |sum w n_i . n| / W, eigenvalues [Q, 3] of every row with enough neighbours, weight [Q] = W).  ``rotate_frame``: u, v turned by that
    angle within the plane (the result must not depend on it)."""
    assert order in (1, 2)
    h = float(np.float32(radius))
    sigma = 0.5 * h if sigma is None else float(sigma)
    floor, default = MIN_NEIGHBORS[order]
    min_nb = default if min_neighbors is None else int(min_neighbors)
    assert min_nb >= floor
    x32 = np.asarray(xyz, np.float32)
    q32 = x32 if query is None else np.asarray(query, np.float32).reshape(-1, 3)
    q = q32.astype(np.float64)
    Q = len(q)
    idx, mask, d = neighbours(x32, q32, h)
    count = mask.sum(1).astype(np.int32)
    w = np.where(mask, np.exp(-(d * d).sum(2) / sigma ** 2), 0.0)
    W = w.sum(1)
    nan1, nan3 = np.full(Q, np.nan), np.full((Q, 3), np.nan)
    out = dict(position=q.copy(), normal=nan3.copy(), mean_curvature=nan1.copy(), gaussian_curvature=nan1.copy(), variation=nan1.copy(),
               count=count, order_used=np.zeros(Q, np.int8), cond=nan1.copy(), pivot_ratio=nan1.copy(), eig_ratio=nan1.copy(),
               sign_margin=nan1.copy(), eigenvalues=nan3.copy(), weight=W)
    if normal is not None and query is None:
        out['normal'] = np.asarray(normal, np.float32).astype(np.float64).copy()
    live = (count >= min_nb) & (W > 0)
    Ws = np.where(live, W, 1.0)
    m = (w[:, :, None] * d).sum(1) / Ws[:, None]
    e = d - m[:, None, :]
    C = np.einsum('qk,qki,qkj->qij', w, e, e)
    C[~live] = np.eye(3)
    val, vec = np.linalg.eigh(C)
    plane = live & (val[:, 1] > np.maximum(RANK_TOL * val[:, 2], ROUNDING_FLOOR * W * h * h))
    n, u, v = vec[:, :, 0].copy(), vec[:, :, 1], vec[:, :, 2]
    if rotate_frame:
        cs, sn = np.cos(rotate_frame), np.sin(rotate_frame)
        u, v = cs * u + sn * v, -sn * u + cs * v
    if normal is not None:
        ni = np.asarray(normal, np.float32).astype(np.float64)[idx]
        s = np.einsum('qk,qki,qi->q', w, ni, n)
        flip = s < 0
        out['sign_margin'] = np.abs(s) / Ws
    else:
        big = np.argmax(np.abs(n), axis=1)              # (the first of the maxima: the lowest axis)
        flip = n[np.arange(Q), big] < 0
    n[flip] *= -1.0
    o = (m * n).sum(1)[:, None] * n
    sel = plane
    out['position'][sel] = (q + o)[sel]
    out['normal'][sel] = n[sel]
    total = val.sum(1)
    out['variation'][sel] = (val[:, 0] / np.where(total > 0, total, 1.0))[sel]
    out['order_used'][sel] = 1
    out['eig_ratio'][sel] = (val[:, 0] / np.where(val[:, 1] > 0, val[:, 1], 1.0))[sel]
    out['eigenvalues'][live] = val[live]
    if order == 1:
        return out
    r = d - o[:, None, :]
    lx, ly, lz = (np.einsum('qki,qi->qk', r, a) / h for a in (u, v, n))
    B = np.stack([np.ones_like(lx), lx, ly, lx * lx, lx * ly, ly * ly], axis=2)
    A = np.einsum('qk,qki,qkj->qij', w, B, B)
    rhs = np.einsum('qk,qki,qk->qi', w, B, lz)
    A[~plane] = np.eye(6)
    a, ok, ratio = cholesky_solve(A, rhs)
    quad = plane & ok
    out['pivot_ratio'][plane] = ratio[plane]
    out['cond'][quad] = np.linalg.cond(A[quad]) if quad.any() else []
    g = n - a[:, 1:2] * u - a[:, 2:3] * v
    g /= np.sqrt((g * g).sum(1))[:, None]
    fx, fy, fxx, fxy, fyy = a[:, 1], a[:, 2], 2 * a[:, 3] / h, a[:, 4] / h, 2 * a[:, 5] / h
    e1 = 1 + fx * fx + fy * fy
    K = (fxx * fyy - fxy * fxy) / e1 ** 2
    H = -((1 + fy * fy) * fxx - 2 * fx * fy * fxy + (1 + fx * fx) * fyy) / (2 * e1 ** 1.5)
    out['position'][quad] = (q + o + (a[:, 0] * h)[:, None] * n)[quad]
    out['normal'][quad] = g[quad]
    out['mean_curvature'][quad] = H[quad]
    out['gaussian_curvature'][quad] = K[quad]
    out['order_used'][quad] = 2
    return out


def smooth_mls(xyz, radius, normal=None, iterations=1, order=2, sigma=None):
    x = np.asarray(xyz, np.float32)
    nrm = None if normal is None else np.asarray(normal, np.float32)
    out_n = nrm
    for _ in range(iterations):
        r = mls_project(x, radius, normal=nrm, order=order, sigma=sigma)
        ok = r['order_used'] > 0
        x = np.where(ok[:, None], r['position'].astype(np.float32), x)
        if nrm is not None:
            nrm = out_n = np.where(ok[:, None], r['normal'].astype(np.float32), nrm)
        else:
            out_n = r['normal'].astype(np.float32)
    return x, out_n


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------------------
SPHERE_N, SPHERE_H, SPHERE_NOISE = 4000, 0.25, 0.01


def _unit_sphere(n, seed):
    rs = np.random.RandomState(seed)
    u = rs.randn(n, 3)
    return u / np.linalg.norm(u, axis=1, keepdims=True), rs


@functools.lru_cache(None)
def noisy_sphere():
    """(xyz float32 [4000, 3] = unit sphere + Gaussian noise 0.01 on every coordinate, normal float32 [4000, 3] = the outward normals of
    the clean points)"""
    u, rs = _unit_sphere(SPHERE_N, 5)
    return (u + SPHERE_NOISE * rs.randn(SPHERE_N, 3)).astype(np.float32), u.astype(np.float32)


@functools.lru_cache(None)
def clean_sphere():
    u, _ = _unit_sphere(SPHERE_N, 6)
    return u.astype(np.float32), u.astype(np.float32)


@functools.lru_cache(None)
def sphere_ref(order, with_normal):
    """the restatement on the noisy sphere, computed once (read-only)"""
    xyz, nrm = noisy_sphere()
    return mls_project(xyz, SPHERE_H, normal=nrm if with_normal else None, order=order)


PLANE_NORMAL = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
PLANE_POINT = np.array([0.1, -0.05, 0.2])
PLANE_H = 0.12


@functools.lru_cache(None)
def tilted_plane():
    """(xyz float32 [2000, 3] on the plane n . (x - p) = 0: a jittered 45 x 45 grid (less 25 points) spanning 1 x 1 in the plane's own axes,
    queries float32 [256, 3]: points over the interior of the patch, up to 0.3 h off the plane)"""
    rs = np.random.RandomState(9)
    a = np.cross(PLANE_NORMAL, [1.0, 0, 0])
    a /= np.linalg.norm(a)
    b = np.cross(PLANE_NORMAL, a)
    gx, gy = np.meshgrid(np.arange(45), np.arange(45), indexing='ij')
    st = (np.stack([gx.ravel(), gy.ravel()], 1) + rs.uniform(-0.4, 0.4, (2025, 2))) / 45.0 - 0.5
    st = st[rs.permutation(2025)[:2000]]
    xyz = PLANE_POINT + st[:, :1] * a + st[:, 1:] * b
    qs = rs.uniform(-0.3, 0.3, (256, 2))
    off = rs.uniform(-0.3, 0.3, (256, 1)) * PLANE_H
    query = PLANE_POINT + qs[:, :1] * a + qs[:, 1:] * b + off * PLANE_NORMAL
    return xyz.astype(np.float32), query.astype(np.float32)


def plane_distance(p):
    return (np.asarray(p, np.float64) - PLANE_POINT) @ PLANE_NORMAL


LATTICE_R = 25                       # in lattice units (segment_ref.UNIT = 2^-10): 3-4-5 multiples put pairs exactly at the radius


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------
def degenerate_clouds():
    """name -> (xyz float32, radius, order, expected order_used of row 0 or None where the restatement decides)"""
    rs = np.random.RandomState(3)
    line = np.stack([np.linspace(-0.1, 0.1, 20), np.zeros(20), np.zeros(20)], 1)
    patch6 = np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0], [-0.05, 0.01, 0], [0.01, -0.05, 0], [0.04, 0.04, 0]], float)
    patch7 = np.concatenate([patch6, [[-0.04, -0.03, 0]]])
    line_plus = np.concatenate([np.stack([np.linspace(-0.1, 0.1, 21), np.zeros(21), np.zeros(21)], 1), [[0.0, 0.03, 0.0]]])
    return {
        'isolated': (np.concatenate([[[5.0, 5.0, 5.0]], rs.uniform(-0.2, 0.2, (50, 3))]), 0.2, 2, 0),
        'collinear': (line, 0.5, 1, 0),
        'coincident': (np.tile([[0.3, -0.2, 0.1]], (30, 1)), 0.1, 1, 0),
        'patch6': (patch6, 0.5, 2, 0),
        'patch7': (patch7, 0.5, 2, 0),
        'line_plus_one': (line_plus, 0.5, 2, None),
        'single': (np.array([[0.1, 0.2, 0.3]]), 0.1, 2, 0),
    }
