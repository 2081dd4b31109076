"""Consistent normal orientation WITHOUT sensor positions (csrc/orient.hip; definition in include/nksr_hip.h).

Hoppe et al. 1992: the minimum spanning forest of the k-nearest-neighbour graph under the weight 1 - |n_i . n_j|, sign flips propagated
along it.  The forest is built by Boruvka rounds that carry a flip parity with every component -- no rooting, no traversal, O(log N)
rounds -- and every edge has a distinct 64-bit integer key, so the forest, and with it every output, is unique and repeats bit for
bit (tests/orient_ref.py restates it with Kruskal in numpy).

  * ``orient_graph(xyz, normal, idx)``: the low-level form on an explicit neighbour table.
  * ``orient_normals(xyz, normal, k)`` / ``CloudIndex.orient_normals``: the table is ``CloudIndex.knn(k, exclude_self=True)``.
  * ``estimate_normals(xyz)``: unoriented kNN-PCA normals (``normals.knn_pca``), then the above; ``preprocess.
    get_estimate_oriented_normal_preprocess_fn`` wraps it for ``Reconstructor.reconstruct``.

A component of the kNN graph that is not connected to the rest is signed on its own: ``seed='+z'`` turns the normal of its highest point
upwards, ``viewpoint=(x, y, z)`` turns the normal of its point nearest the viewpoint towards it.

CHUNKED RECONSTRUCTION.  Orientation is a property of the whole cloud.  Under ``reconstruct(..., chunk_size > 0)`` a ``preprocess_fn``
runs per chunk, and the open piece of surface inside a chunk cannot be signed by the '+z' rule (its highest point may look either way),
so chunks would disagree.  Call ``estimate_normals`` on the whole cloud first and pass ``normal=``.  GPU tensors only."""
import collections

import torch

from . import cloud_input, ops
from ._lib import ORIENT_MAX_K, ORIENT_SEED_VIEWPOINT, ORIENT_SEED_Z, call, ptr, stream

OrientedNormals = collections.namedtuple('OrientedNormals', 'normal flipped component n_components')
# normal float32 [N, 3]; flipped uint8 [N] (1: the input normal was negated); component int32 [N], dense ids in the order of every
# component's minimum point index; n_components int

_NORMAL_LIMIT = 2.0 ** 60           # three products of components below it cannot overflow fp32: the dot is finite


def _seed_args(seed, viewpoint):
    if viewpoint is not None:
        v = [float(c) for c in (viewpoint.tolist() if torch.is_tensor(viewpoint) else viewpoint)]
        if len(v) != 3 or not all(abs(c) < float('inf') for c in v):
            raise ValueError('orient: viewpoint must be three finite numbers (got %r)' % (viewpoint,))
        return ORIENT_SEED_VIEWPOINT, v
    if seed != '+z':
        raise ValueError("orient: seed must be '+z' (got %r); pass viewpoint=(x, y, z) for the other rule" % (seed,))
    return ORIENT_SEED_Z, [0.0, 0.0, 0.0]


def _check_k(k, n, what):
    k = int(k)
    if k < 1 or k > ORIENT_MAX_K:
        raise ValueError('%s: 1 <= k <= %d (got %d)' % (what, ORIENT_MAX_K, k))
    if n * k >= 1 << 32:
        raise ValueError('%s: N * k = %d slots do not fit 32 bits' % (what, n * k))
    return k


def _check_cloud(xyz, normal, what):
    """float32 contiguous xyz / normal [N, 3] on one GPU, finite (one readback)"""
    xyz, normal = cloud_input.points(xyz, what), cloud_input.points(normal, what, 'normal')
    cloud_input.rows_like(normal, xyz.shape[0], xyz.device, what, 'normal')
    if xyz.shape[0]:
        amax = torch.stack([xyz.abs().max(), normal.abs().max()]).tolist()
        if not amax[0] < float('inf'):
            raise RuntimeError('%s: non-finite coordinates in the input' % what)
        if not amax[1] < _NORMAL_LIMIT:                     # also catches NaN / inf
            raise RuntimeError('%s: normals must be finite, every component below 2^60 in magnitude' % what)
    return xyz, normal


def _timed(stats, stage, fn):
    """fn(), its time added to stats[stage] (HIP events; one synchronisation per stage: only the profiling tool passes stats)"""
    if stats is None:
        return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    stats[stage] = stats.get(stage, 0.0) + a.elapsed_time(b)
    return out


def _forest(normal, idx, order=None, stats=None):
    """The Boruvka rounds: -> (rep int32 [N] = one representative per component, par uint8 [N] = the sign of every point relative to
    its representative).  One readback per round: (links made, points still active)."""
    n, k, dev = idx.shape[0], idx.shape[1], idx.device
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    par = torch.empty(n, dtype=torch.uint8, device=dev)
    done = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.int64, device=dev)             # (the kernels read it as uint64)
    link = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    lpar = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    counters = torch.empty(2, dtype=torch.int32, device=dev)
    st = stream()
    call('nksr_orient_init', n, ptr(rep), ptr(par), ptr(done), ptr(best), st)
    components = n
    if stats is not None:
        stats['rounds'] = []
    while components > 1:
        counters.zero_()
        _timed(stats, 'propose', lambda: call('nksr_orient_propose', ptr(normal), ptr(idx), n, k, ptr(order), ptr(rep), ptr(done), ptr(best),
                                              ptr(counters), st))
        _timed(stats, 'hook', lambda: call('nksr_orient_hook', ptr(normal), ptr(idx), n, k, ptr(rep), ptr(par), ptr(best), ptr(link[0]),
                                           ptr(lpar[0]), ptr(counters), st))
        hooks, active = counters.tolist()
        if stats is not None:
            stats['rounds'].append({'components': components, 'active_points': active, 'links': hooks})
        if hooks == 0:
            break
        cur = 0
        for _ in range((hooks - 1).bit_length()):           # a chain of links is at most `hooks` long: ceil(log2) doublings flatten it
            _timed(stats, 'jump', lambda: call('nksr_orient_jump', ptr(rep), n, ptr(link[cur]), ptr(lpar[cur]), ptr(link[1 - cur]),
                                               ptr(lpar[1 - cur]), st))
            cur = 1 - cur
        _timed(stats, 'relabel', lambda: call('nksr_orient_relabel', n, ptr(rep), ptr(par), ptr(link[cur]), ptr(lpar[cur]), ptr(best), st))
        components -= hooks
    return rep, par


def orient_graph(xyz, normal, idx, seed='+z', viewpoint=None, order=None, stats=None):
    """Orients ``normal`` [N, 3] along the minimum spanning forest of the graph ``idx`` [N, k] (integer; row i lists neighbours of point
    i; an entry < 0, >= N or equal to i is ignored, duplicates are allowed; 1 <= k <= 32, N k < 2^32).  -> ``OrientedNormals``.
    ``seed`` / ``viewpoint``: the rule that fixes the sign of every connected component (module docstring).  ``order`` (int32 [N], a
    permutation): the order in which the kernels visit the points -- it changes nothing in the result; a Morton order keeps the lanes
    of a wavefront inside one component (``CloudIndex.orient_normals`` passes the grid's).  A zero normal is legal: its edges weigh 1 and
    flip nothing.  ``stats`` (a dict; tools/prof_orient.py): filled with the time of every stage in ms and, under 'rounds', the
    components / active points / links of every round, at the price of a synchronisation per stage."""
    mode, v = _seed_args(seed, viewpoint)
    xyz, normal = _check_cloud(xyz, normal, 'orient_graph')
    n, dev = xyz.shape[0], xyz.device
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.shape[0] != n or idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise RuntimeError('orient_graph: idx must be an integer [N,k] tensor')
    if idx.device != dev:
        raise RuntimeError('orient_graph: idx is on %s, the cloud on %s' % (idx.device, dev))
    k = _check_k(idx.shape[1], n, 'orient_graph')
    if n == 0:
        return OrientedNormals(normal, torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int32, device=dev), 0)
    if idx.dtype != torch.int32:                            # (what does not fit int32 is no point index: -1 is ignored like it)
        idx = torch.where((idx >= 0) & (idx < n), idx, torch.full_like(idx, -1)).to(torch.int32)
    idx = idx.contiguous()
    if order is not None:
        if order.shape != (n,) or order.device != dev:
            raise RuntimeError('orient_graph: order must be an [N] tensor on the device of xyz')
        order = order.to(torch.int32).contiguous()
    rep, par = _forest(normal, idx, order, stats)
    seed_key = torch.zeros(n, dtype=torch.int64, device=dev)
    min_index = torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
    flipped = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty_like(normal)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n + 1, dtype=torch.int32, device=dev)
    st = stream()

    def seeds():
        call('nksr_orient_seeds', ptr(xyz), n, ptr(rep), mode, v[0], v[1], v[2], ptr(seed_key), ptr(min_index), st)
        call('nksr_orient_apply', ptr(xyz), ptr(normal), n, ptr(rep), ptr(par), ptr(seed_key), ptr(min_index), mode, v[0], v[1], v[2],
             ptr(flipped), ptr(out), ptr(parent), ptr(flags), st)
    _timed(stats, 'seeds', seeds)
    rank = ops.exclusive_sum_i32(flags)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    call('nksr_uf_labels', ptr(parent), n, ptr(rank), ptr(label), st)
    return OrientedNormals(out, flipped, label, int(rank[n].item()))


def _orient_on_index(index, normal, k, seed, viewpoint, stats=None):
    k = _check_k(k, index.n, 'orient_normals')
    if k + 1 > index.n:
        raise ValueError('orient_normals: k = %d other points of a cloud of %d points' % (k, index.n))
    _seed_args(seed, viewpoint)                                             # (argument errors before the search)
    cloud_input.rows_like(normal, index.n, None, 'orient_normals', 'normal')
    idx, _ = _timed(stats, 'knn', lambda: index.knn(k, exclude_self=True))
    return orient_graph(index.xyz, normal, idx.to(torch.int32), seed=seed, viewpoint=viewpoint, order=index.pg.perm, stats=stats)


def orient_normals(xyz, normal, k=16, seed='+z', viewpoint=None):
    """``orient_graph`` on the k nearest other points of every point (``CloudIndex(xyz).knn(k, exclude_self=True)``).
    k + 1 <= N; an empty cloud gives empty results."""
    from .cloud import CloudIndex
    _seed_args(seed, viewpoint)
    xyz, normal = _check_cloud(xyz, normal, 'orient_normals')
    if xyz.shape[0] == 0:
        _check_k(k, 0, 'orient_normals')
        return orient_graph(xyz, normal, torch.empty((0, int(k)), dtype=torch.int32, device=xyz.device), seed=seed, viewpoint=viewpoint)
    if int(k) + 1 > xyz.shape[0]:
        _check_k(k, xyz.shape[0], 'orient_normals')
        raise ValueError('orient_normals: k = %d other points of a cloud of %d points' % (int(k), xyz.shape[0]))
    return _orient_on_index(CloudIndex(xyz), normal, k, seed, viewpoint)


def estimate_normals(xyz, knn=64, orient_k=16, seed='+z', viewpoint=None):
    """(xyz', normal') of a cloud that has positions only: unoriented kNN-PCA normals (``normals.knn_pca``, ``knn`` neighbours, the
    point itself included), the points whose neighbourhood the kernel marks invalid dropped, the rest -- in the caller's order --
    oriented by ``orient_normals(k=orient_k)``.  Fewer than ``knn`` (or ``orient_k + 1``) points: ``normals.TooFewPoints``.
    For chunked reconstruction run this on the WHOLE cloud and pass ``normal=`` (module docstring)."""
    from .normals import TooFewPoints, knn_pca
    knn, orient_k = int(knn), int(orient_k)
    _seed_args(seed, viewpoint)                                             # (argument errors first)
    xyz = cloud_input.points(xyz, 'estimate_normals')
    if knn < 3:
        raise ValueError('estimate_normals: knn must be at least 3 (got %d)' % knn)
    _check_k(orient_k, xyz.shape[0], 'estimate_normals')
    if xyz.shape[0] < max(knn, orient_k + 1):
        raise TooFewPoints('need at least knn=%d and orient_k + 1 = %d points' % (knn, orient_k + 1))
    pg, nrm, _, valid = knn_pca(xyz, knn)
    keep = valid > 0
    order = torch.argsort(pg.perm[keep])                                   # back to the caller's order
    xs, ns = pg.xyz[keep][order].contiguous(), nrm[keep][order].contiguous()
    if xs.shape[0] < orient_k + 1:
        raise TooFewPoints('only %d points have a valid neighbourhood: orient_k + 1 = %d are needed' % (xs.shape[0], orient_k + 1))
    return xs, orient_normals(xs, ns, k=orient_k, seed=seed, viewpoint=viewpoint).normal
