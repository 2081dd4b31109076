"""Global registration of point clouds on the GPU: FPFH features, feature matching, RANSAC over matched pairs (surfaced as
``nksr.cloud.compute_fpfh_feature``, ``match_features``, ``registration_ransac_based_on_feature_matching`` and ``register_global``;
names follow Open3D).

``cloud.icp`` refines a pose that is nearly right; this module FINDS one for scans that share no frame -- two handheld sweeps, two tiles
of different sessions -- and hands it to the ICP.

  * ``compute_fpfh_feature`` / ``CloudIndex.compute_fpfh_feature``: a Fast Point Feature Histogram (Rusu 2009) per point: 3 x 11 bins
    of the angles between the normals of a point and of its neighbours (csrc/fpfh.hip ``k_spfh``: integer counts), then the
    distance-weighted sum over the neighbours' histograms (``k_fpfh``: fp64 in a fixed order).  include/nksr_hip.h states every
    operation; no atomics, the same call gives the same bits.
  * ``match_features``: the nearest feature of the other cloud by brute force (csrc/global_register.hip ``k_feature_match``: direct
    fp32 differences, the lowest index on a tie).
  * ``registration_ransac_based_on_feature_matching``: index triples drawn on the host (``draw_triples``), rejected where their edge
    lengths disagree (``edge_length_keep``), fitted by batched Kabsch in fp64 numpy (``fit_triples``); ALL surviving poses scored on the
    device (``k_hypothesis_score`` of csrc/score_dev.h: integer counts), the best refitted once on its inliers (``k_corr_accumulate`` + ``nksr_icp_reduce`` +
    ``register.kabsch_step``).
  * ``register_global``: voxel downsampling, features, RANSAC and point-to-plane ICP in one call.
``draw_triples``, ``edge_length_keep`` and ``fit_triples`` are plain numpy and need no GPU.  Everything else: GPU tensors only.
"""
import numpy as np
import torch

from . import _lib, cloud_input
from ._lib import call, ptr, require_gpu, stream

BINS, MAX_K = _lib.FPFH_BINS, _lib.FPFH_MAX_K
MATCH_MAX_PAIRS = 1 << 34           # rows of A x rows of B one match call takes (131 072 x 131 072): the search is brute force
SCORE_BATCH = 1 << 16               # hypotheses per nksr_pose_score launch (6 MB of transforms)
assert SCORE_BATCH <= _lib.POSE_MAX_H


class FpfhFeature:
    """``data`` float32 [N, 33] = the features; ``spfh_count`` int32 [N, 33] = the simplified histograms as counts; ``n_neighbours`` int32
    [N] = the neighbours that took part.  What they were computed from, in the caller's order: ``neighbour_idx`` int32 [N, max_nn],
    ``neighbour_d2`` float32 [N, max_nn] (squared, as the kNN kernel wrote them), ``neighbour_mask`` int32 [N] (bit m: neighbour m took
    part)."""

    def __init__(self, data, spfh_count, n_neighbours, neighbour_idx, neighbour_d2, neighbour_mask):
        self.data, self.spfh_count, self.n_neighbours = data, spfh_count, n_neighbours
        self.neighbour_idx, self.neighbour_d2, self.neighbour_mask = neighbour_idx, neighbour_d2, neighbour_mask

    def __len__(self):
        return int(self.data.shape[0])

    def __repr__(self):
        return 'FpfhFeature(%d points, %d bins)' % (self.data.shape[0], self.data.shape[1])


class RansacResult:
    """``transformation`` float64 [4, 4] CPU tensor (source -> target); ``fitness`` / ``inlier_rmse``: ``evaluate_registration`` of the two
    clouds at that pose and ``max_correspondence_distance`` (what they mean for ICP); ``correspondence_set`` int64 [C, 2] on the device
    = the matched (source, target) pairs the poses were drawn from and scored on; ``n_drawn`` = triples without a repeated index,
    ``n_scored`` = those that passed the edge-length test; ``best_hypothesis`` = the number of the winning draw (0 ..
    ``max_iteration`` - 1), ``best_count`` = the pairs within the distance at the pose returned; ``refined`` = the refit was kept."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondence_set, n_drawn, n_scored, best_hypothesis, best_count, refined):
        self.transformation, self.fitness, self.inlier_rmse, self.correspondence_set = transformation, fitness, inlier_rmse, correspondence_set
        self.n_drawn, self.n_scored, self.best_hypothesis, self.best_count, self.refined = n_drawn, n_scored, best_hypothesis, best_count, refined

    def __repr__(self):
        return 'RansacResult(fitness=%.6g, inlier_rmse=%.6g, best_count=%d of %d pairs, scored %d of %d draws)' % (
            self.fitness, self.inlier_rmse, self.best_count, self.correspondence_set.shape[0], self.n_scored, self.n_drawn)


# ---- the host side of RANSAC: plain numpy, no GPU ----------------------------------------------------------------------------------------
def draw_triples(n_corr, max_iteration, seed=0):
    """-> (triples int64 [M, 3], draw int64 [M]): ``numpy.random.default_rng(seed).integers(0, n_corr, (max_iteration, 3))`` without the
    rows that repeat an index; ``draw`` = the row every triple had (its hypothesis number)."""
    n_corr, max_iteration = int(n_corr), int(max_iteration)
    if n_corr < 1 or max_iteration < 1:
        raise ValueError('draw_triples: n_corr and max_iteration must be >= 1 (got %d, %d)' % (n_corr, max_iteration))
    t = np.random.default_rng(seed).integers(0, n_corr, size=(max_iteration, 3), dtype=np.int64)
    keep = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    return t[keep], np.nonzero(keep)[0].astype(np.int64)


def edge_length_keep(src, tgt, edge_length_threshold):
    """bool [M]: ``src`` / ``tgt`` float64 [M, 3, 3] = the three source points of every triple and their partners.  A triple is dropped
    if one of its edges (0-1, 1-2, 2-0) is shorter among the source points than ``edge_length_threshold`` times the same edge among
    the target points, or the other way round."""
    src, tgt, thr = np.asarray(src, np.float64), np.asarray(tgt, np.float64), float(edge_length_threshold)
    keep = np.ones(src.shape[0], dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ls = np.sqrt(((src[:, a] - src[:, b]) ** 2).sum(1))
        lt = np.sqrt(((tgt[:, a] - tgt[:, b]) ** 2).sum(1))
        keep &= (ls >= thr * lt) & (lt >= thr * ls)
    return keep


def fit_triples(src, tgt):
    """float64 [M, 3, 4]: per row the rigid motion (R | t) that takes ``src`` [M, n, 3] onto ``tgt`` [M, n, 3] in the least-squares sense
    (Kabsch: SVD of the centred moment matrix with the determinant correction, so no reflection comes back)."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    if src.shape[0] == 0:
        return np.zeros((0, 3, 4))
    mp, mq = src.mean(1), tgt.mean(1)
    H = np.einsum('mia,mib->mab', src - mp[:, None], tgt - mq[:, None])
    U, _, Vt = np.linalg.svd(H)
    V, Ut = np.swapaxes(Vt, 1, 2), np.swapaxes(U, 1, 2)
    d = np.sign(np.linalg.det(V @ Ut))
    D = np.zeros_like(H)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = np.where(d != 0, d, 1.0)
    R = V @ D @ Ut
    t = mq - np.einsum('mab,mb->ma', R, mp)
    return np.concatenate([R, t[:, :, None]], axis=2)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def _unit_normals(normal, n, device):
    cloud_input.rows_like(normal, n, device, None, 'normal', floating=True)
    m = normal.double()
    length = m.norm(dim=1, keepdim=True)
    if n and not (float(length.min()) > 0.0 and float(length.max()) < float('inf')):
        raise ValueError('compute_fpfh_feature: normals must be finite and not zero')
    return (m / length).float().contiguous()


def _features(f, what):
    f = f.data if isinstance(f, FpfhFeature) else f
    if not torch.is_tensor(f) or f.dim() != 2 or f.shape[1] != BINS or not f.is_floating_point():
        raise RuntimeError('%s must be an FpfhFeature or a floating-point [N, %d] tensor' % (what, BINS))
    require_gpu(f.device)
    return f.to(torch.float32).contiguous()


# ---- the kernels, one call each ------------------------------------------------------------------------------------------------------------
def spfh(xyz, normal, idx, d2, radius):
    """``nksr_spfh`` -> (count int32 [N, 33], n_neighbours int32 [N], mask int32 [N]).  ``xyz`` / ``normal`` float32 [N, 3] (unit normals),
    ``idx`` int32 [N, k] into the same order, ``d2`` float32 [N, k]."""
    n, k, dev = xyz.shape[0], idx.shape[1], xyz.device
    count = torch.empty((n, BINS), dtype=torch.int32, device=dev)
    nn = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_spfh', ptr(xyz), ptr(normal), n, ptr(idx), ptr(d2), k, radius, ptr(count), ptr(nn), ptr(mask), stream())
    return count, nn, mask


def fpfh(count, n_neighbours, mask, idx, d2):
    """``nksr_fpfh`` -> float32 [N, 33]"""
    n, k = count.shape[0], idx.shape[1]
    out = torch.empty((n, BINS), dtype=torch.float32, device=count.device)
    call('nksr_fpfh', ptr(count), ptr(n_neighbours), ptr(mask), n, ptr(idx), ptr(d2), k, ptr(out), stream())
    return out


def feature_match(a, b):
    """``nksr_feature_match`` -> (idx int32 [Na] = the nearest row of ``b`` for every row of ``a`` or -1, dist2 float32 [Na])."""
    na, nb, dev = a.shape[0], b.shape[0], a.device
    if na * nb > MATCH_MAX_PAIRS:
        raise ValueError('match_features: %d x %d features are more than the %d pairs one brute-force search takes; thin the clouds '
                         'with cloud.voxel_downsample first' % (na, nb, MATCH_MAX_PAIRS))
    idx = torch.empty(na, dtype=torch.int32, device=dev)
    dist2 = torch.empty(na, dtype=torch.float32, device=dev)
    keys = torch.empty(na, dtype=torch.int64, device=dev)
    call('nksr_feature_match', ptr(a), na, ptr(b) if nb else None, nb, ptr(keys), ptr(idx), ptr(dist2), stream())
    return idx, dist2


def pose_scores(src, tgt, transforms, threshold):
    """int32 [H] on the device: for every transform of ``transforms`` (float64 [H, 3, 4] or [H, 12], numpy or tensor) the number of pairs
    (``src`` [C, 3], ``tgt`` [C, 3], float32) with |R p + t - q| <= ``threshold`` (fp64, no fused multiply-add); -1 for a transform that is
    not finite.  Launches of at most 65 536 hypotheses."""
    T = torch.as_tensor(transforms, dtype=torch.float64).reshape(-1, 12)
    h, dev = T.shape[0], src.device
    counts = torch.empty(h, dtype=torch.int32, device=dev)
    for lo in range(0, h, SCORE_BATCH):
        part = T[lo:lo + SCORE_BATCH].to(dev).contiguous()
        call('nksr_pose_score', ptr(src), ptr(tgt), src.shape[0], ptr(part), part.shape[0], threshold, counts.data_ptr() + 4 * lo, stream())
    return counts


def corr_sums(src, tgt, transform, centre, threshold):
    """``nksr_corr_accumulate`` + ``nksr_icp_reduce`` for ONE transform (float64 [3, 4] or [4, 4]) -> (mask uint8 [C] on the device, sums
    float64 numpy [NKSR_ICP_FIELDS], the point method's layout: one 256-byte read)."""
    from .register import RowSums
    c, dev = src.shape[0], src.device
    rows = RowSums(c, 12, dev)
    rows.set(np.asarray(transform, np.float64)[:3], centre)
    mask = torch.empty(c, dtype=torch.uint8, device=dev)
    call('nksr_corr_accumulate', ptr(src), ptr(tgt), c, rows.args_ptr, rows.centre_ptr, threshold, ptr(mask), ptr(rows.partials), stream())
    return mask, rows.reduce()


# ---- features ------------------------------------------------------------------------------------------------------------------------------
def fpfh_on_index(index, normal, radius, max_nn=32):
    """``compute_fpfh_feature`` on a ``cloud.CloudIndex``."""
    radius, max_nn = cloud_input.positive(radius, 'compute_fpfh_feature', 'radius'), int(max_nn)
    if max_nn < 1 or max_nn > MAX_K:
        raise ValueError('compute_fpfh_feature: 1 <= max_nn <= %d (got %d)' % (MAX_K, max_nn))
    normal = _unit_normals(normal, index.n, index.device)
    idx64, d2 = index.knn_d2(max_nn, exclude_self=True)
    idx = idx64.to(torch.int32).contiguous()
    count, nn, mask = spfh(index.xyz, normal, idx, d2, radius)
    return FpfhFeature(fpfh(count, nn, mask, idx, d2), count, nn, idx, d2, mask)


def compute_fpfh_feature(xyz, normal, radius, max_nn=32, index=None):
    """FPFH of every point of ``xyz`` [N, 3] with ``normal`` [N, 3] (finite; scaled to unit length on the way in) -> ``FpfhFeature``.
    The neighbours of a point are its ``max_nn`` nearest other points (1 <= max_nn <= 32 < N) that lie within ``radius``: Open3D's
    hybrid search.  The cloud should be voxel-downsampled so that ``radius`` holds about ``max_nn`` points -- radius ~ 3 voxels --:
    in a denser cloud the ``max_nn`` nearest points cover a part of the radius only and the feature describes a smaller patch than
    meant.  ``index``: a ``CloudIndex`` of ``xyz`` built before."""
    from .cloud import CloudIndex
    if index is None:
        index = CloudIndex(cloud_input.points(xyz, None))
    elif index.n != xyz.shape[0]:
        raise ValueError('compute_fpfh_feature: the index holds %d points, xyz %d' % (index.n, xyz.shape[0]))
    return fpfh_on_index(index, normal, radius, max_nn)


# ---- matching ------------------------------------------------------------------------------------------------------------------------------
def match_features(source_feature, target_feature, mutual_filter=False):
    """-> (idx int64 [Ns], dist2 float32 [Ns], mutual bool [Ns]).  ``idx[a]`` = the target feature nearest source feature a: the smallest
    sum_j (s_j - t_j)^2 in fp32 (ascending j), the lowest index among equals; -1 (dist2 +inf) for a source row that is not finite or an
    empty target.  ``mutual[a]``: source a is in turn the nearest of target ``idx[a]`` (a second launch, target to source).
    ``mutual_filter``: ``idx`` is -1 wherever ``mutual`` is False.  At most 2^34 pairs of rows per call."""
    a, b = _features(source_feature, 'source_feature'), _features(target_feature, 'target_feature')
    if a.device != b.device:
        raise RuntimeError('source_feature is on %s, target_feature on %s' % (a.device, b.device))
    idx, dist2 = feature_match(a, b)
    back, _ = feature_match(b, a)
    idx = idx.long()
    here = torch.arange(a.shape[0], device=a.device)
    mutual = (idx >= 0) & (back.long()[idx.clamp(min=0)] == here) if b.shape[0] else torch.zeros_like(here, dtype=torch.bool)
    if mutual_filter:
        idx = torch.where(mutual, idx, torch.full_like(idx, -1))
    return idx, dist2, mutual


# ---- RANSAC --------------------------------------------------------------------------------------------------------------------------------
def ransac_hypotheses(src_pairs, tgt_pairs, max_iteration, edge_length_threshold, seed):
    """The poses RANSAC scores, from the matched pairs on the host (float [C, 3] numpy each) -> (transforms float64 [M, 3, 4], draw int64
    [M], n_drawn): ``draw_triples``, ``edge_length_keep``, ``fit_triples``."""
    s64, t64 = np.asarray(src_pairs, np.float64), np.asarray(tgt_pairs, np.float64)
    triples, draw = draw_triples(len(s64), max_iteration, seed)
    keep = edge_length_keep(s64[triples], t64[triples], edge_length_threshold)
    triples, kept = triples[keep], draw[keep]
    return fit_triples(s64[triples], t64[triples]), kept, len(draw)


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, max_correspondence_distance,
                                                  mutual_filter=True, ransac_n=3, edge_length_threshold=0.9, max_iteration=100000, seed=0,
                                                  refine=True):
    """A pose for ``source`` [Ns, 3] on ``target`` [Nt, 3] from their features (``FpfhFeature`` or [N, 33] tensors) -> ``RansacResult``.

    1. ``match_features`` pairs every source point with a target point; with ``mutual_filter`` and at least ``ransac_n`` mutual matches
       only those are kept.  2. ``max_iteration`` index triples of pairs are drawn (``numpy.random.default_rng(seed)``), those with a
       repeated index dropped.  3. A triple is dropped if an edge among its source points and the same edge among its target points
       differ by more than the factor ``edge_length_threshold``.  4. The rest are fitted by Kabsch in fp64 on the host (the pairs are
       read back once).  5. Every pose is scored on the device: the pairs within ``max_correspondence_distance``.  6. The highest count
       wins, the earliest draw on a tie.  7. ``refine``: one least-squares refit on the winner's inliers, kept if its count is not
       lower.  Fewer than ``ransac_n`` pairs, or no triple that survives: RuntimeError."""
    from .register import evaluate_registration, kabsch_step
    if int(ransac_n) != 3:
        raise ValueError('registration_ransac_based_on_feature_matching: ransac_n must be 3 (got %r)' % (ransac_n,))
    thr = cloud_input.positive(max_correspondence_distance, 'registration_ransac_based_on_feature_matching', 'max_correspondence_distance')
    max_iteration = int(max_iteration)
    if max_iteration < 1:
        raise ValueError('registration_ransac_based_on_feature_matching: max_iteration must be >= 1 (got %d)' % max_iteration)
    source, target = cloud_input.points(source, None, 'source'), cloud_input.points(target, None, 'target')
    fs, ft = _features(source_feature, 'source_feature'), _features(target_feature, 'target_feature')
    if fs.shape[0] != source.shape[0] or ft.shape[0] != target.shape[0]:
        raise ValueError('registration_ransac_based_on_feature_matching: %d / %d features for %d / %d points' % (
            fs.shape[0], ft.shape[0], source.shape[0], target.shape[0]))
    if mutual_filter:
        idx, _, mutual = match_features(fs, ft)
        keep = mutual if int(mutual.sum()) >= 3 else idx >= 0
    else:
        idx = feature_match(fs, ft)[0].long()
        keep = idx >= 0
    ci = torch.nonzero(keep).flatten()
    cj = idx[ci]
    if ci.numel() < 3:
        raise RuntimeError('registration_ransac_based_on_feature_matching: %d correspondences, fewer than ransac_n = 3' % ci.numel())
    src_pairs, tgt_pairs = source[ci].contiguous(), target[cj].contiguous()
    pairs = torch.stack([src_pairs, tgt_pairs]).cpu().numpy()                   # one gather of the pairs, read back once
    transforms, draw, n_drawn = ransac_hypotheses(pairs[0], pairs[1], max_iteration, edge_length_threshold, seed)
    if len(draw) == 0:
        raise RuntimeError('registration_ransac_based_on_feature_matching: none of the %d triples drawn (%d without a repeated index) '
                           'survives the edge-length test at %g' % (max_iteration, n_drawn, edge_length_threshold))
    counts = pose_scores(src_pairs, tgt_pairs, transforms, thr).cpu().numpy()
    best = int(np.argmax(counts))                       # (the first of the maxima: the earliest draw)
    if counts[best] < 0:
        raise RuntimeError('registration_ransac_based_on_feature_matching: no finite pose among the %d hypotheses' % len(draw))
    T = np.eye(4)
    T[:3] = transforms[best]
    best_count, refined = int(counts[best]), False
    if refine:
        t64 = pairs[1].astype(np.float64)
        centre = 0.5 * (t64.min(0) + t64.max(0))
        _, sums = corr_sums(src_pairs, tgt_pairs, T, centre, thr)
        M = kabsch_step(sums, centre)
        if M is not None:
            T2 = M @ T
            T2[3] = [0.0, 0.0, 0.0, 1.0]
            c2 = int(pose_scores(src_pairs, tgt_pairs, T2[None, :3], thr).cpu()[0]) if np.all(np.isfinite(T2)) else -1
            if c2 >= best_count:
                T, best_count, refined = T2, c2, True
    ev = evaluate_registration(source, target, thr, T)
    return RansacResult(torch.from_numpy(T.copy()), ev.fitness, ev.inlier_rmse, torch.stack([ci, cj], dim=1), n_drawn, len(draw),
                        int(draw[best]), best_count, refined)


# ---- the usual recipe ----------------------------------------------------------------------------------------------------------------------
def register_global(source, target, voxel_size, source_normal=None, target_normal=None, seed=0, refine_icp=True, **ransac_kwargs):
    """Register ``source`` [Ns, 3] onto ``target`` [Nt, 3] whatever their poses: 1. ``voxel_downsample`` of both clouds at ``voxel_size``
    with their normals (``cloud.estimate_normals(knn=32)`` where none are given; the points it drops are dropped here);
    2. ``compute_fpfh_feature`` at radius 3 ``voxel_size``; 3. ``registration_ransac_based_on_feature_matching`` at 1.5 ``voxel_size``
    (``ransac_kwargs`` go there); 4. with ``refine_icp``, ``icp(method='plane')`` on the FULL clouds at 1.5 ``voxel_size`` from that
    pose.  -> the result of the last stage (``IcpResult``, or ``RansacResult`` without ICP) with the RANSAC result as ``.ransac``."""
    from . import cloud
    voxel_size = cloud_input.positive(voxel_size, 'register_global', 'voxel_size')
    clouds = []
    for xyz, normal, what in ((source, source_normal, 'source'), (target, target_normal, 'target')):
        xyz = cloud_input.points(xyz, None, what)
        if normal is None:
            xyz, normal = cloud.estimate_normals(xyz, knn=32)
        down = cloud.voxel_downsample(xyz, voxel_size, normal=normal)
        clouds.append((xyz, normal, down, compute_fpfh_feature(down.xyz, down.normal, 3.0 * voxel_size)))
    (src, _, sd, sf), (tgt, tgt_normal, td, tf) = clouds
    ransac = registration_ransac_based_on_feature_matching(sd.xyz, td.xyz, sf, tf, 1.5 * voxel_size, seed=seed, **ransac_kwargs)
    result = ransac
    if refine_icp:
        result = cloud.icp(src, tgt, 1.5 * voxel_size, init=ransac.transformation, method='plane', target_normal=tgt_normal)
    result.ransac = ransac
    return result
