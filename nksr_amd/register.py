"""Rigid registration of point clouds on the GPU: ICP (surfaced as ``nksr.cloud.icp`` and friends; names follow Open3D).

Scans of one scene whose poses are a little off give the solve two parallel sheets; ``icp`` brings a source cloud onto a target
before the clouds are merged and handed to ``Reconstructor.reconstruct``.

  * ``icp`` / ``CloudIndex.icp``: point-to-point (Kabsch) or point-to-plane (linearised, Gauss-Newton) iterations.  One pass =
    csrc/register.hip ``k_icp_accumulate`` (transform, nearest target point within the radius on a ``PointGrid``, fp64 terms of the
    normal equations, per-workgroup sums in a fixed order) + ``k_icp_reduce``: no floating-point atomics, the same call gives the same
    bits.  The 6-parameter solve runs on the host in fp64 numpy (``kabsch_step`` / ``plane_step``): ONE device-to-host read of the
    ``NKSR_ICP_FIELDS`` = 32 doubles (256 bytes) of sums per pass, nothing else leaves the GPU.
  * ``evaluate_registration``: one pass, no update.
  * ``icp_multiscale``: coarse to fine over ``voxel_downsample``.
  * ``apply_transform``: fp64 arithmetic, rounded once to fp32.
GPU tensors only.  A transformation is a float64 [4, 4] CPU tensor that maps source coordinates to target coordinates.
"""
import math

import numpy as np
import torch

from . import _lib, cloud_input, ops
from ._lib import call, ptr, stream

FIELDS, BLOCK = _lib.ICP_FIELDS, _lib.ICP_BLOCK
COUNT, D2 = _lib.ICP_COUNT, _lib.ICP_D2
PT_P, PT_Q, PT_PQ = _lib.ICP_PT_P, _lib.ICP_PT_Q, _lib.ICP_PT_PQ
PL_JJ, PL_JR, PL_RR = _lib.ICP_PL_JJ, _lib.ICP_PL_JR, _lib.ICP_PL_RR
METHODS = {'point': 0, 'plane': 1}
MIN_CORRESPONDENCES = {'point': 3, 'plane': 6}


class IcpResult:
    """``transformation`` float64 [4, 4] CPU tensor (source -> target); ``fitness`` = the share of source points with a target point
    within the distance; ``inlier_rmse`` = the root mean square Euclidean distance of those pairs (0 without any);
    ``correspondence_set`` int64 [N] on the device = the target point (caller's order) of every source point, -1 = none;
    ``iterations`` = the updates applied; ``converged``; ``pass_sums`` = the sums of every pass (float64 numpy [NKSR_ICP_FIELDS] each,
    layout: include/nksr_hip.h), the last one belonging to ``transformation`` like fitness, rmse and the correspondences."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondence_set, iterations, converged, pass_sums):
        self.transformation, self.fitness, self.inlier_rmse = transformation, fitness, inlier_rmse
        self.correspondence_set, self.iterations, self.converged, self.pass_sums = correspondence_set, iterations, converged, pass_sums

    def __repr__(self):
        return 'IcpResult(fitness=%.6g, inlier_rmse=%.6g, iterations=%d, converged=%s)' % (self.fitness, self.inlier_rmse, self.iterations,
                                                                                         self.converged)


# ---- the host side of an iteration: small pure functions of the sums (fp64 numpy) ----------------------------------------------------
def rodrigues(w):
    """exp([w]x): the rotation by |w| radians about w / |w|."""
    w = np.asarray(w, np.float64)
    th2 = float(w @ w)
    th = math.sqrt(th2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-4:                    # sin(t) / t and (1 - cos(t)) / t^2 by their series: the quotients lose digits here
        a, b = 1.0 - th2 / 6.0 + th2 * th2 / 120.0, 0.5 - th2 / 24.0 + th2 * th2 / 720.0
    else:
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    return np.eye(3) + a * K + b * (K @ K)


def _about(R, t, centre):
    """4 x 4 of x -> R (x - c) + c + t"""
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = centre - R @ centre + t
    return M


def kabsch(H):
    """The rotation R that maximises trace(R H) for H = sum p q^T (p is turned onto q): SVD with the determinant correction, so a
    reflection never comes back (coplanar or noisy input)."""
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T


def kabsch_step(sums, centre):
    """Point-to-point update from the moment sums (about ``centre``): the rigid motion, as a 4 x 4 in world coordinates, that takes
    the transformed source points onto their correspondences in the least-squares sense.  None: fewer than 3 correspondences."""
    sums, centre = np.asarray(sums, np.float64), np.asarray(centre, np.float64)
    n = sums[COUNT]
    if not n >= MIN_CORRESPONDENCES['point']:
        return None
    mp, mq = sums[PT_P:PT_P + 3] / n, sums[PT_Q:PT_Q + 3] / n
    H = sums[PT_PQ:PT_PQ + 9].reshape(3, 3) - n * np.outer(mp, mq)
    if not np.all(np.isfinite(H)):
        return None
    R = kabsch(H)
    return _about(R, mq - R @ mp, centre)


def plane_system(sums):
    """(A [6, 6], b [6]) = (sum J J^T, sum J r) of the plane method's sums."""
    sums = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    iu = np.triu_indices(6)
    A[iu] = sums[PL_JJ:PL_JJ + 21]
    A = A + np.triu(A, 1).T
    return A, sums[PL_JR:PL_JR + 6].copy()


def plane_step(sums, centre):
    """Point-to-plane update: xi = (omega, v) solves (sum J J^T) xi = -sum J r by Cholesky; the motion is x -> exp([omega]x) (x - c)
    + c + v.  None: fewer than 6 correspondences, or a system Cholesky rejects (flat or otherwise unconstrained geometry)."""
    sums, centre = np.asarray(sums, np.float64), np.asarray(centre, np.float64)
    if not sums[COUNT] >= MIN_CORRESPONDENCES['plane']:
        return None
    A, b = plane_system(sums)
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    xi = -np.linalg.solve(L.T, np.linalg.solve(L, b))
    if not np.all(np.isfinite(xi)):
        return None
    return _about(rodrigues(xi[:3]), xi[3:], centre)


STEPS = {'point': kabsch_step, 'plane': plane_step}


def fitness_rmse(sums, n_src):
    n = float(sums[COUNT])
    return n / n_src, (math.sqrt(max(float(sums[D2]), 0.0) / n) if n > 0 else 0.0)


def stop_rule(fit, rmse, prev_fit, prev_rmse, relative_fitness, relative_rmse):
    return abs(fit - prev_fit) <= relative_fitness * prev_fit and abs(rmse - prev_rmse) <= relative_rmse * prev_rmse


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def check_transformation(T, what='init'):
    """-> float64 numpy [4, 4]; None = identity.  ValueError unless finite, 4 x 4, bottom row (0, 0, 0, 1)."""
    if T is None:
        return np.eye(4)
    if torch.is_tensor(T):
        T = T.detach().cpu().numpy()
    try:
        T = np.array(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s must be a 4 x 4 matrix' % what)
    if T.shape != (4, 4):
        raise ValueError('%s must be a 4 x 4 matrix (got shape %s)' % (what, T.shape))
    if not np.all(np.isfinite(T)):
        raise ValueError('%s has non-finite entries' % what)
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError('%s: the bottom row must be (0, 0, 0, 1)' % what)
    return T


def _check_source(source, device):
    source = cloud_input.points(source, None, 'source', finite=True)
    if source.device != device:
        raise RuntimeError('source is on %s, the target on %s' % (source.device, device))
    if source.shape[0] < 1:
        raise ValueError('icp: empty source')
    return source


def _target_index(target):
    from . import cloud
    if isinstance(target, cloud.CloudIndex):
        return target
    if torch.is_tensor(target) and target.dim() == 2 and target.shape[0] == 0:
        raise ValueError('icp: empty target')
    return cloud.CloudIndex(target)


def _check_method(method, target_normal, index):
    if method not in METHODS:
        raise ValueError("icp: method must be 'point' or 'plane' (got %r)" % (method,))
    if method == 'point':
        return None
    if target_normal is None:
        raise ValueError("icp: method='plane' needs target_normal")
    cloud_input.rows_like(target_normal, index.n, index.device, 'icp', 'target_normal')
    return target_normal.to(torch.float32)


# ---- transforms ------------------------------------------------------------------------------------------------------------------------
def apply_transform(xyz, transformation, normal=None):
    """``xyz`` [N, 3] moved by the 4 x 4 ``transformation``: fp64 arithmetic, rounded once to fp32.  With ``normal`` [N, 3] ->
    (xyz, normal): normals take the rotation only."""
    T = check_transformation(transformation, 'transformation')
    cloud_input.rows3(xyz, None)
    _lib.require_gpu(xyz.device)
    Td = torch.from_numpy(T).to(xyz.device)
    out = (xyz.double() @ Td[:3, :3].t() + Td[:3, 3]).float()
    if normal is None:
        return out
    cloud_input.rows_like(normal, xyz.shape[0], xyz.device, None, 'normal')
    return out, (normal.double() @ Td[:3, :3].t()).float()


# ---- one pass ------------------------------------------------------------------------------------------------------------------------
# Source order.  Neighbouring lanes should walk the same cells, so the source is sorted ONCE by its cell key at the initial pose (the
# pose moves little afterwards) and the correspondences are mapped back at the end.  Measured on one MI355X at 1 M x 1 M rounded-box
# points (profiles/register_icp.md): the accumulate kernel takes 0.43 ms sorted against 1.54 ms in the caller's order at radius 0.01
# (42 points per cell) and 5.8 against 25.4 ms at radius 0.05 (1 025 per cell); the sort costs 0.58 ms once per call, less than the
# first pass saves.  The sort stays.
SORT_SOURCE = True


class RowSums:
    """The device side of one pass of fixed-order sums over ``n`` items (``block_row_sums`` of csrc/icp_dev.h + ``nksr_icp_reduce``):
    ``args`` = float64 [n_args + 3], the kernel's arguments followed by the centre the sums are taken about; ``partials`` = one row of
    ``NKSR_ICP_FIELDS`` per workgroup of the accumulate kernel, which the owner launches between ``set`` and ``reduce``; ``sums``."""

    def __init__(self, n, n_args, device):
        self.nrows = (n + BLOCK - 1) // BLOCK
        self.args = torch.empty(n_args + 3, dtype=torch.float64, device=device)
        self.args_ptr, self.centre_ptr = self.args.data_ptr(), self.args.data_ptr() + 8 * n_args
        self.partials = torch.empty((self.nrows, FIELDS), dtype=torch.float64, device=device)
        self.sums = torch.empty(FIELDS, dtype=torch.float64, device=device)

    def set(self, args, centre):
        self.args.copy_(torch.from_numpy(np.concatenate([np.asarray(args, np.float64).reshape(-1), np.asarray(centre, np.float64)])))

    def reduce(self):
        """-> the sums as float64 numpy [NKSR_ICP_FIELDS]: the pass's one device-to-host read (256 bytes)"""
        call('nksr_icp_reduce', ptr(self.partials), self.nrows, ptr(self.sums), stream())
        return self.sums.cpu().numpy()


class IcpPass:
    """Everything one (target, source, radius, method) needs on the device; ``run(T)`` -> the sums of the pass at ``T`` (float64 numpy,
    the pass's only device-to-host read)."""

    def __init__(self, index, source, radius, method, target_normal, init, sort_source=None):
        self.index, self.radius, self.method = index, radius, METHODS[method]
        dev = index.device
        g = self.grid = index._radius_grid(radius)
        self.normal = g.to_grid(target_normal) if target_normal is not None else None
        self.centre = index.bbox_centre()
        n = self.n = source.shape[0]
        self.order = None
        if SORT_SOURCE if sort_source is None else sort_source:
            lim = ((1 << 20) - 8) * g.cell * 0.5          # (a pose far outside the key range: any order will do, the keys must exist)
            at_init = apply_transform(source, init).nan_to_num(0.0, lim, -lim).clamp(-lim, lim).contiguous()
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            call('nksr_point_keys', ptr(at_init), n, g.inv_cell, ptr(keys), stream())
            _, order = ops.sort_pairs(keys, torch.arange(n, dtype=torch.int32, device=dev))
            self.order = order.long()
            source = source[self.order].contiguous()
        self.source = source
        self.rows = RowSums(n, 12, dev)                                        # the transform's 12
        self.corr = torch.empty(n, dtype=torch.int64, device=dev)

    def run(self, T):
        from .neighbours import _grid_args
        g, rows = self.grid, self.rows
        rows.set(T[:3], self.centre)
        call('nksr_icp_accumulate', ptr(g.xyz), self.index.n, *_grid_args(g), ptr(g.perm), ptr(self.normal), ptr(self.source), self.n,
             rows.args_ptr, rows.centre_ptr, self.radius, self.method, ptr(self.corr), ptr(rows.partials), stream())
        return rows.reduce()

    def correspondences(self):
        """of the last pass, in the caller's source order"""
        if self.order is None:
            return self.corr.clone()
        out = torch.empty_like(self.corr)
        out[self.order] = self.corr
        return out


def _prepare(source, target, max_correspondence_distance, init, method, target_normal, what):
    index = _target_index(target)
    source = _check_source(source, index.device)
    radius = cloud_input.positive(max_correspondence_distance, 'icp', 'max_correspondence_distance')
    normal = _check_method(method, target_normal, index)
    T = check_transformation(init, what)
    return IcpPass(index, source, radius, method, normal, T), T


def icp(source, target, max_correspondence_distance, init=None, method='point', target_normal=None, max_iteration=30,
        relative_fitness=1e-6, relative_rmse=1e-6):
    """Register ``source`` [N, 3] onto ``target`` ([M, 3], or a ``CloudIndex`` so that one target serves many sources) -> ``IcpResult``.

    Pass i evaluates T_i (T_0 = ``init``, identity by default): every source point moved by T_i is paired with its nearest target
    point within ``max_correspondence_distance`` (inclusive), and the pairs give T_{i+1} -- ``method='point'``: the rigid motion that
    minimises sum |p - q|^2 (Kabsch); ``method='plane'``: one Gauss-Newton step on sum (n_q . (p - q))^2 with ``target_normal`` [M, 3].
    The loop stops (``converged=True``) when |fitness_i - fitness_{i-1}| <= relative_fitness * fitness_{i-1} and the same holds for
    the rmse, or after ``max_iteration`` updates (``converged=False``; one more pass then evaluates the last transformation: fitness,
    rmse and correspondences always belong to the transformation returned).  No correspondences, fewer than 3 (point) / 6 (plane) of
    them, or a plane system that Cholesky rejects end the loop with ``converged=False`` and the transformation as it was.

    Each pass reads 256 bytes (the 32 fp64 sums) back to the host, where the 6-parameter solve runs; the clouds stay on the GPU."""
    max_iteration = int(max_iteration)
    if max_iteration < 0:
        raise ValueError('icp: max_iteration must be >= 0 (got %d)' % max_iteration)
    ps, T = _prepare(source, target, max_correspondence_distance, init, method, target_normal, 'init')
    step = STEPS[method]
    history, converged, updates = [], False, 0
    prev = None
    while True:
        sums = ps.run(T)
        history.append(sums)
        fit, rmse = fitness_rmse(sums, ps.n)
        if prev is not None and stop_rule(fit, rmse, prev[0], prev[1], relative_fitness, relative_rmse):
            converged = True
            break
        if updates == max_iteration:
            break
        M = step(sums, ps.centre)
        if M is None:
            break
        T = M @ T
        T[3] = [0.0, 0.0, 0.0, 1.0]
        updates += 1
        prev = (fit, rmse)
    return IcpResult(torch.from_numpy(T.copy()), fit, rmse, ps.correspondences(), updates, converged, history)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, method='point', target_normal=None):
    """One pass at ``transformation`` (identity by default), no update -> ``IcpResult`` (``iterations`` 0, ``converged`` False): what
    pass 0 of ``icp`` with ``init=transformation`` sees."""
    ps, T = _prepare(source, target, max_correspondence_distance, transformation, method, target_normal, 'transformation')
    sums = ps.run(T)
    fit, rmse = fitness_rmse(sums, ps.n)
    return IcpResult(torch.from_numpy(T.copy()), fit, rmse, ps.correspondences(), 0, False, [sums])


def icp_multiscale(source, target, voxel_sizes, max_correspondence_distances, max_iterations, init=None, method='point',
                   target_normal=None, relative_fitness=1e-6, relative_rmse=1e-6):
    """Coarse to fine: level l runs ``icp`` on both clouds thinned by ``voxel_downsample(..., voxel_sizes[l])`` (mean positions; mean
    normals, scaled back to unit length, serve ``method='plane'``) with ``max_correspondence_distances[l]`` and
    ``max_iterations[l]``, seeded with the result of the level before (the first with ``init``).  A voxel size of None or 0 takes the
    clouds as they are.  ``target`` is a tensor here.  -> the ``IcpResult`` of the last level: its fitness, rmse and correspondences
    refer to that level's clouds (use ``evaluate_registration`` for the full ones)."""
    from . import cloud
    levels = list(zip(list(voxel_sizes), list(max_correspondence_distances), list(max_iterations)))
    if not levels or not (len(levels) == len(list(voxel_sizes)) == len(list(max_correspondence_distances)) == len(list(max_iterations))):
        raise ValueError('icp_multiscale: voxel_sizes, max_correspondence_distances and max_iterations must be equally long, not empty')
    if not torch.is_tensor(target):
        raise RuntimeError('icp_multiscale: target must be a [M,3] tensor (every level builds its own index)')
    if method not in METHODS:
        raise ValueError("icp: method must be 'point' or 'plane' (got %r)" % (method,))
    if method == 'plane' and target_normal is None:
        raise ValueError("icp: method='plane' needs target_normal")
    T = check_transformation(init, 'init')
    result = None
    for voxel, radius, iters in levels:
        if voxel:
            src = cloud.voxel_downsample(source, voxel).xyz
            tgt = cloud.voxel_downsample(target, voxel, normal=target_normal if method == 'plane' else None)
            tgt_xyz, tgt_n = tgt.xyz, tgt.normal
        else:
            src, tgt_xyz, tgt_n = source, target, target_normal if method == 'plane' else None
        result = icp(src, tgt_xyz, radius, init=T, method=method, target_normal=tgt_n, max_iteration=iters,
                     relative_fitness=relative_fitness, relative_rmse=relative_rmse)
        T = result.transformation.numpy()
    return result
