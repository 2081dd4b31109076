"""float64 numpy / scipy restatement of nksr_amd/register.py + csrc/register.hip (ICP), and the standard inputs of its tests.

Nearest neighbours come from a cKDTree over the target, residuals and sums from plain float64 arithmetic, the updates from the
correspondences themselves (centred points for Kabsch, the stacked Jacobian for point-to-plane, scipy's rotation vector for the
exponential) rather than from the packed sums, so that ``register.kabsch_step`` / ``plane_step`` are checked against something they
do not share code with.  The sum layouts are written out here by hand (include/nksr_hip.h states them)."""
import functools

import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

FIELDS = 32
COUNT, D2, PT_P, PT_Q, PT_PQ, PL_JJ, PL_JR, PL_RR = 0, 1, 2, 5, 8, 2, 23, 29


# ---- standard inputs --------------------------------------------------------------------------------------------------------------------
def rigid(axis, degrees, translation=(0.0, 0.0, 0.0)):
    axis = np.asarray(axis, np.float64)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.radians(degrees) * axis / np.linalg.norm(axis)).as_matrix()
    T[:3, 3] = translation
    return T


T_STAR = rigid((1.0, 2.0, 3.0), 5.0, (0.02, -0.015, 0.01))
RADIUS = 0.05


def move(T, xyz):
    """float64 T x, rounded once to fp32"""
    return (np.asarray(xyz, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def standard_inputs():
    """-> dict: target [6000, 3] / normal (rounded box, seed 0), source_a (4000 fresh samples, seed 1) and source_b (a random
    4000-subset of the target, permuted), both moved by the inverse of T_STAR and rounded to fp32."""
    from nksr_amd import utils
    target, normal = utils.synth_rounded_box(6000, seed=0)
    fresh, _ = utils.synth_rounded_box(4000, seed=1)
    subset = np.random.RandomState(2).permutation(6000)[:4000]
    inv = np.linalg.inv(T_STAR)
    return {'target': target, 'normal': normal, 'source_a': move(inv, fresh), 'source_b': move(inv, target[subset]), 'subset': subset}


def pose_error(T, T_true=T_STAR):
    """(rotation error in radians, translation error) of T against T_true"""
    dR = T[:3, :3] @ T_true[:3, :3].T
    return float(np.linalg.norm(Rotation.from_matrix(dR).as_rotvec())), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def bbox_centre(target):
    t = np.asarray(target, np.float64)
    return 0.5 * (t.min(0) + t.max(0))


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------
def transform(T, source):
    """p = R s + t in float64, in the order the kernel states: ((T0 x + T1 y) + T2 z) + T3 per row"""
    s = np.asarray(source, np.float32).astype(np.float64)
    return np.stack([((T[a, 0] * s[:, 0] + T[a, 1] * s[:, 1]) + T[a, 2] * s[:, 2]) + T[a, 3] for a in range(3)], axis=1)


def nearest_within(p, target, radius, tree=None):
    """-> (index [N] or -1, nearest distance, second-nearest distance): the search point is fl32(p) (as float64), the radius
    fl32(radius), inclusive."""
    t64 = np.asarray(target, np.float32).astype(np.float64)
    tree = tree if tree is not None else cKDTree(t64)
    p32 = p.astype(np.float32).astype(np.float64)
    k = min(2, t64.shape[0])
    d, i = tree.query(p32, k=k)
    d, i = d.reshape(len(p), k), i.reshape(len(p), k)
    d1 = d[:, 0]
    d2 = d[:, 1] if k == 2 else np.full(len(p), np.inf)
    r = float(np.float32(radius))
    idx = np.where(d1 * d1 <= float(np.float32(r) * np.float32(r)), i[:, 0], -1)
    return idx, d1, d2


def decided(d1, d2, radius):
    """rows whose answer does not hang on rounding: nearest and second nearest differ by more than 1e-5 relative, and the nearest
    is not within 1e-5 r of the radius"""
    return (np.abs(d2 - d1) > 1e-5 * np.maximum(d2, 1e-300)) & (np.abs(d1 - radius) > 1e-5 * radius)


def terms(method, p, target, corr, centre, normal=None):
    """[N, FIELDS] float64: the terms of every source point (zero rows where corr < 0), formed as include/nksr_hip.h states them"""
    out = np.zeros((len(p), FIELDS))
    m = corr >= 0
    q = np.asarray(target, np.float32).astype(np.float64)[corr[m]]
    pm = p[m]
    d = pm - q
    pp = pm - centre
    t = np.zeros((int(m.sum()), FIELDS))
    t[:, COUNT] = 1.0
    t[:, D2] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    if method == 'point':
        qq = q - centre
        for a in range(3):
            t[:, PT_P + a] = pp[:, a]
            t[:, PT_Q + a] = qq[:, a]
            for b in range(3):
                t[:, PT_PQ + 3 * a + b] = pp[:, a] * qq[:, b]
    else:
        n = np.asarray(normal, np.float32).astype(np.float64)[corr[m]]
        r = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        J = [pp[:, 1] * n[:, 2] - pp[:, 2] * n[:, 1], pp[:, 2] * n[:, 0] - pp[:, 0] * n[:, 2], pp[:, 0] * n[:, 1] - pp[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2]]
        k = PL_JJ
        for a in range(6):
            for b in range(a, 6):
                t[:, k] = J[a] * J[b]
                k += 1
            t[:, PL_JR + a] = J[a] * r
        t[:, PL_RR] = r * r
    out[m] = t
    return out


def sums(method, p, target, corr, centre, normal=None):
    return terms(method, p, target, corr, centre, normal).sum(axis=0)


# ---- the updates, from the correspondences themselves -------------------------------------------------------------------------------------
def point_step(p, q):
    """4 x 4 of the rigid motion that minimises sum |M p - q|^2; None with fewer than 3 pairs"""
    if len(p) < 3:
        return None
    mp, mq = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - mp).T @ (q - mq))
    D = np.eye(3)
    D[2, 2] = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    M = np.eye(4)
    M[:3, :3] = Vt.T @ D @ U.T
    M[:3, 3] = mq - M[:3, :3] @ mp
    return M


def plane_step(p, q, n, centre):
    """one Gauss-Newton step on sum (n . (p + w x (p - c) + v - q))^2: x -> exp([w]x) (x - c) + c + v; None with fewer than 6 pairs or a
    normal matrix that is not positive definite"""
    if len(p) < 6:
        return None
    J = np.concatenate([np.cross(p - centre, n), n], axis=1)
    r = np.einsum('ij,ij->i', n, p - q)
    A, b = J.T @ J, J.T @ r
    if np.linalg.eigvalsh(A).min() <= 0:
        return None
    xi = -np.linalg.solve(A, b)
    M = np.eye(4)
    M[:3, :3] = Rotation.from_rotvec(xi[:3]).as_matrix()
    M[:3, 3] = centre - M[:3, :3] @ centre + xi[3:]
    return M


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
def icp(source, target, radius, init=None, method='point', normal=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> dict(transformation, fitness, inlier_rmse, correspondence_set, iterations, converged, history = the T of every pass)"""
    t64 = np.asarray(target, np.float32).astype(np.float64)
    n64 = np.asarray(normal, np.float32).astype(np.float64) if normal is not None else None
    tree, centre = cKDTree(t64), bbox_centre(target)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    prev, updates, converged, history = None, 0, False, []
    while True:
        history.append(T.copy())
        p = transform(T, source)
        idx, d1, _ = nearest_within(p, target, radius, tree)
        m = idx >= 0
        cnt = int(m.sum())
        q = t64[idx[m]]
        fit = cnt / len(p)
        rmse = float(np.sqrt(((p[m] - q) ** 2).sum() / cnt)) if cnt else 0.0
        if prev is not None and abs(fit - prev[0]) <= relative_fitness * prev[0] and abs(rmse - prev[1]) <= relative_rmse * prev[1]:
            converged = True
            break
        if updates == max_iteration:
            break
        M = point_step(p[m], q) if method == 'point' else plane_step(p[m], q, n64[idx[m]], centre)
        if M is None:
            break
        T = M @ T
        updates += 1
        prev = (fit, rmse)
    return {'transformation': T, 'fitness': fit, 'inlier_rmse': rmse, 'correspondence_set': idx, 'iterations': updates,
            'converged': converged, 'history': history}
