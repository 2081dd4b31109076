"""float64 / float32 numpy restatement of csrc/fpfh.hip and csrc/global_register.hip, operation by operation as include/nksr_hip.h
states them, the RANSAC loop of nksr_amd/global_register.py around them, and the standard inputs of their tests.

Every function takes what the kernel takes (the neighbour lists included: the GPU tests hand over the GPU's own, so neighbour ties
play no part) and gives what the kernel gives.  The drawing, the edge-length test and the triple fit are the plain numpy functions of
nksr_amd/global_register.py themselves (they ARE the host side); matching, scoring and the refit are restated here."""
import functools

import numpy as np

import register_ref

BINS = 33
RADIUS, MAX_NN, DISTANCE, DRAWS, SEED = 0.15, 32, 0.03, 30000, 0
T_STAR = register_ref.rigid((1.0, 2.0, 3.0), 140.0, (0.7, -0.4, 0.3))
EPS = 1e-9


# ---- standard inputs ---------------------------------------------------------------------------------------------------------------------
def standard_shape(n=1200, seed=0):
    """(xyz, normal) float32: a rounded box of n points, a sphere and a torus of n / 3 each, placed so that nothing is symmetric"""
    from nksr_amd import utils
    parts = [utils.synth_rounded_box(n, seed=seed), utils.synth_sphere(n // 3, radius=0.13, seed=seed, center=(0.24, 0.14, 0.12)),
             utils.synth_torus(n // 3, R=0.12, r=0.04, seed=seed, center=(-0.15, -0.05, 0.19))]
    return np.concatenate([p[0] for p in parts]).astype(np.float32), np.concatenate([p[1] for p in parts]).astype(np.float32)


def move_cloud(T, xyz, normal):
    return register_ref.move(T, xyz), (np.asarray(normal, np.float64) @ T[:3, :3].T).astype(np.float32)


@functools.lru_cache(maxsize=None)
def standard_inputs(n=1200):
    """target (seed 0) and source (seed 1, moved by the inverse of T_STAR), with their analytic normals"""
    tx, tn = standard_shape(n, 0)
    sx, sn = standard_shape(n, 1)
    sx, sn = move_cloud(np.linalg.inv(T_STAR), sx, sn)
    return {'target': tx, 'target_normal': tn, 'source': sx, 'source_normal': sn}


def partial_scans(n=1200, band=0.15):
    """the standard shape cut by the oblique plane x + y + z = 0, either half with ``band`` beyond it (examples/recons_registered.py);
    the second half in the frame T_STAR^-1"""
    ax, an = standard_shape(n, 0)
    bx, bn = standard_shape(n, 1)
    side = np.ones(3) / np.sqrt(3.0)
    ka, kb = ax @ side < band, bx @ side > -band
    bx, bn = move_cloud(np.linalg.inv(T_STAR), bx[kb], bn[kb])
    return {'target': ax[ka], 'target_normal': an[ka], 'source': bx, 'source_normal': bn}


def knn(xyz, k):
    """(idx int32 [N, k], d2 float32 [N, k]) of the k nearest other points, for the tests that run without a GPU"""
    from scipy.spatial import cKDTree
    x = np.asarray(xyz, np.float32).astype(np.float64)
    _, i = cKDTree(x).query(x, k=k + 1)
    idx = np.empty((len(x), k), np.int64)
    for r in range(len(x)):             # the point itself out of its row (duplicates may come before it)
        row = i[r][i[r] != r]
        idx[r] = row[:k]
    d = (x[idx] - x[:, None]).astype(np.float32)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return idx.astype(np.int32), d2.astype(np.float32)


# ---- SPFH --------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _bin(f, shift, width):
    b = np.floor((11.0 * (f + shift)) / width)
    return np.where(b >= 10.0, 10, np.where(b >= 0.0, b, 0)).astype(np.int64)


def _bins(f0, f1, f2):
    return np.stack([_bin(f0, np.pi, 2.0 * np.pi), _bin(f1, 1.0, 2.0), _bin(f2, 1.0, 2.0)], axis=-1)


def _branch(swap, ni, nj, d, a1, a2):
    """(f0, f1, f2, the cross product is not zero) of every pair taken from j's side (swap) or from i's"""
    s = swap[..., None]
    u, o, dd = np.where(s, nj, ni), np.where(s, ni, nj), np.where(s, -d, d)
    f2 = np.where(swap, -a2, a1)
    v = _cross(dd, u)
    nonzero = (v != 0.0).any(-1)
    v = v / np.sqrt(_dot(v, v))[..., None]
    w = _cross(u, v)
    return np.arctan2(_dot(w, o), _dot(u, o)), _dot(v, o), f2, nonzero


def pair_features(xyz, normal, idx, d2, radius):
    """Everything about the pairs (i, idx[i, m]): dict of [N, k] arrays -- ``part`` (takes part), ``bins`` [N, k, 3], ``undecided``."""
    x, nrm = np.asarray(xyz, np.float32).astype(np.float64), np.asarray(normal, np.float32).astype(np.float64)
    idx, d2 = np.asarray(idx, np.int64), np.asarray(d2, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    near = (d2 <= r2) & (d2 > 0)
    with np.errstate(all='ignore'):
        ni, nj = np.broadcast_to(nrm[:, None], nrm[idx].shape), nrm[idx]
        d = x[idx] - x[:, None]
        L = np.sqrt(_dot(d, d))
        a1, a2 = _dot(ni, d) / L, _dot(nj, d) / L
        swap = np.abs(a1) < np.abs(a2)
        f0, f1, f2, nz = _branch(swap, ni, nj, d, a1, a2)
        bins = _bins(f0, f1, f2)
        part = near & nz
        und = np.zeros_like(part)
        for k, f in enumerate((f0, f1, f2)):
            for e in (-EPS, EPS):
                moved = [f0, f1, f2]
                moved[k] = f + e
                und |= (_bins(*moved) != bins).any(-1)
        und |= np.pi - np.abs(f0) <= EPS                    # f0 is an angle: -pi and pi are one place, bins 0 and 10 meet there
        und &= nz                                           # (a pair that takes no part has no bins to change)
        g0, g1, g2, gz = _branch(~swap, ni, nj, d, a1, a2)
        und |= (np.abs(np.abs(a1) - np.abs(a2)) <= EPS) & ((gz != nz) | (nz & (_bins(g0, g1, g2) != bins).any(-1)))
    return {'part': part, 'bins': bins, 'undecided': und & near}


def spfh(xyz, normal, idx, d2, radius):
    """-> (count int32 [N, 33], n_neighbours int32 [N], mask uint32 [N], undecided rows bool [N])"""
    pf = pair_features(xyz, normal, idx, d2, radius)
    n, k = pf['part'].shape
    count = np.zeros((n, BINS), np.int32)
    rows = np.arange(n)
    for m in range(k):
        on = pf['part'][:, m]
        for g in range(3):
            np.add.at(count, (rows[on], 11 * g + pf['bins'][on, m, g]), 1)
    mask = (pf['part'].astype(np.uint64) << np.arange(k, dtype=np.uint64)).sum(1).astype(np.uint32)
    return count, pf['part'].sum(1).astype(np.int32), mask, undecided(pf, idx)


def undecided(pf, idx):
    """rows whose histogram (or that of a neighbour that takes part, which the FPFH reads) hangs on a rounding: a pair is undecided when
    moving one of f0, f1, f2 by +-1e-9 changes a bin, or when ||a1| - |a2|| <= 1e-9 and the other swap branch changes one"""
    own = pf['undecided'].any(1)
    return own | (own[np.asarray(idx, np.int64)] & pf['part']).any(1)


# ---- FPFH --------------------------------------------------------------------------------------------------------------------------------
def fpfh(count, n_neighbours, mask, idx, d2):
    count, nn = np.asarray(count, np.float64), np.asarray(n_neighbours, np.int64)
    mask, idx, d2 = np.asarray(mask).astype(np.uint32), np.asarray(idx, np.int64), np.asarray(d2, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        S = np.where(nn[:, None] > 0, count * (100.0 / nn.astype(np.float64))[:, None], 0.0)
        F = np.zeros_like(S)
        for m in range(idx.shape[1]):
            on = ((mask >> np.uint32(m)) & np.uint32(1)).astype(bool)
            F = np.where(on[:, None], F + S[idx[:, m]] / d2[:, m, None], F)
        for g in range(3):
            s = np.zeros(len(F))
            for b in range(11 * g, 11 * g + 11):
                s = s + F[:, b]
            F[:, 11 * g:11 * g + 11] = np.where((s > 0)[:, None], F[:, 11 * g:11 * g + 11] * (100.0 / s)[:, None], F[:, 11 * g:11 * g + 11])
    return (F + S).astype(np.float32)


def compute_fpfh(xyz, normal, radius=RADIUS, max_nn=MAX_NN):
    """the whole feature on the host (its own neighbour search): dict(data, count, n, mask, idx, d2, undecided)"""
    idx, d2 = knn(xyz, max_nn)
    count, nn, mask, und = spfh(xyz, normal, idx, d2, radius)
    return {'data': fpfh(count, nn, mask, idx, d2), 'count': count, 'n': nn, 'mask': mask, 'idx': idx, 'd2': d2, 'undecided': und}


# ---- matching ------------------------------------------------------------------------------------------------------------------------------
def match(A, B):
    """-> (idx int32 [Na], dist2 float32 [Na]): fp32 differences, products and sums in ascending j, the lowest index among equals; -1 and
    +inf where no distance is finite"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    if B.shape[0] == 0:
        return np.full(A.shape[0], -1, np.int32), np.full(A.shape[0], np.inf, np.float32)
    D = np.zeros((A.shape[0], B.shape[0]), np.float32)
    with np.errstate(all='ignore'):
        for j in range(A.shape[1]):
            d = A[:, j, None] - B[None, :, j]
            D = D + d * d
    D = np.where(np.isfinite(D), D, np.float32(np.inf))
    idx = np.argmin(D, axis=1)
    best = D[np.arange(len(A)), idx]
    return np.where(np.isfinite(best), idx, -1).astype(np.int32), best.astype(np.float32)


def mutual(idx_ab, idx_ba):
    ok = idx_ab >= 0
    return ok & (idx_ba[np.where(ok, idx_ab, 0)] == np.arange(len(idx_ab)))


# ---- scoring and the sums ----------------------------------------------------------------------------------------------------------------
def pose_inliers(src, tgt, T, threshold):
    """(bool [C], the moved points float64 [C, 3]) for one transform [3 or 4, 4]"""
    p = register_ref.transform(np.asarray(T, np.float64), src)
    e = p - np.asarray(tgt, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= threshold * threshold, p


def pose_counts(src, tgt, transforms, threshold):
    T = np.asarray(transforms, np.float64).reshape(-1, 3, 4)
    out = np.empty(len(T), np.int32)
    for h in range(len(T)):
        out[h] = pose_inliers(src, tgt, T[h], threshold)[0].sum() if np.all(np.isfinite(T[h])) else -1
    return out


def corr_terms(src, tgt, T, centre, threshold):
    """(mask bool [C], terms float64 [C, 32]: the point method's rows of register_ref.terms over the inliers)"""
    m, p = pose_inliers(src, tgt, T, threshold)
    corr = np.where(m, np.arange(len(m)), -1)
    return m, register_ref.terms('point', p, tgt, corr, np.asarray(centre, np.float64))


# ---- RANSAC --------------------------------------------------------------------------------------------------------------------------------
def ransac(source, target, fs, ft, distance=DISTANCE, mutual_filter=True, edge_length_threshold=0.9, max_iteration=DRAWS, seed=SEED,
           refine=True):
    """the loop of global_register.registration_ransac_based_on_feature_matching on the host -> dict"""
    from nksr_amd import global_register as gr
    idx, _ = match(fs, ft)
    keep = idx >= 0
    if mutual_filter:
        mu = mutual(idx, match(ft, fs)[0])
        keep = mu if mu.sum() >= 3 else keep
    ci = np.nonzero(keep)[0]
    cj = idx[ci].astype(np.int64)
    sp, tp = np.asarray(source, np.float32)[ci], np.asarray(target, np.float32)[cj]
    transforms, draw, n_drawn = gr.ransac_hypotheses(sp, tp, max_iteration, edge_length_threshold, seed)
    counts = pose_counts(sp, tp, transforms, distance)
    best = int(np.argmax(counts))
    T = np.eye(4)
    T[:3] = transforms[best]
    best_count, refined = int(counts[best]), False
    if refine:
        m, p = pose_inliers(sp, tp, T, distance)
        M = register_ref.point_step(p[m], tp[m].astype(np.float64))
        if M is not None:
            T2 = M @ T
            c2 = int(pose_counts(sp, tp, T2[None, :3], distance)[0])
            if c2 >= best_count:
                T, best_count, refined = T2, c2, True
    return {'transformation': T, 'pairs': np.stack([ci, cj], axis=1), 'n_drawn': n_drawn, 'n_scored': len(draw), 'best_hypothesis': int(draw[best]),
            'best_count': best_count, 'refined': refined, 'counts': counts}
