"""Time of point-cloud segmentation (nksr_amd/segment.py; csrc/segment.hip) and of its parts.

    python -m nksr_amd.tools.prof_segment [--n 1000000] [--eps 0.005 0.01 0.05] [--min-points 10] [--planes 1000] [--reps 9]
                                          [--no-host] [--json OUT]
    python -m nksr_amd.tools.prof_segment --resources       (no GPU needed: compiles csrc/segment.hip and prints what the compiler reports
                                                             for its kernels -- registers, spills, LDS, occupancy)

Input: ``utils.synth_rounded_box``, n points (seed 0).  HIP events around the launches, a host clock around what ends in a
synchronise; every figure is the median of --reps warm runs with the smallest and largest next to it.

DBSCAN, per eps (the grid is ``CloudIndex._radius_grid(eps)``):
  grid            the PointGrid of the radius (keys, sort, cell ranges, hash): once per (index, eps)
  core            nksr_radius_count(cap = min_points): the core flags
  count_uncapped  nksr_radius_count without a cap on the same grid: the same loads as the hook kernel and no unions -- the floor
                  the hook kernel is compared against; timed alternately with `components`
  components      nksr_dbscan_components: k_uf_init + k_dbscan_hook<first> + k_dbscan_shorten + k_dbscan_hook<all> + k_uf_flatten
  init_flatten    k_uf_init + k_uf_flatten on a forest nothing was hooked in (nksr_uf_components without pairs): what of
                  `components` is not the hook kernel, at the least
  min_caller      nksr_dbscan_min_caller
  border          nksr_dbscan_border
  stats           segment.cluster_stats: sort by label, runs, cloud.voxel_reduce;  stats_reduce: the voxel_reduce call in it alone
  total           CloudIndex.cluster_dbscan with the grid built (host clock)
  host            scipy on the host: core flags by cKDTree.query_ball_point(return_length, 16 workers), pairs by query_pairs (the API
                  has no worker argument: one core), scipy.sparse.csgraph.connected_components on the core-core pairs; one run, the
                  tree build apart.  Left out where the pair list would not fit (more than --max-pairs pairs, from the GPU's count).
Plane RANSAC on the same cloud, --planes hypotheses:
  sample          segment.sample_planes (the gather of 3 H points and its read-back; host clock)
  score           nksr_plane_score, all hypotheses in one launch
  moments         nksr_plane_moments;  reduce: nksr_icp_reduce over its rows
  total           segment_plane (host clock)
  numpy_score     the same counts in float64 numpy on the host, one run; they must equal the GPU's
"""
import argparse
import json
import os
import time

import numpy as np

from .prof_register import _clock, _events, kernel_resources


def host_dbscan(x64, tree, eps, min_points):
    """-> (seconds by part, number of clusters)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = {}
    t0 = time.perf_counter()
    core = tree.query_ball_point(x64, eps, workers=min(16, os.cpu_count() or 1), return_length=True) >= min_points
    t['core'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    pairs = tree.query_pairs(eps, output_type='ndarray')
    t['query_pairs'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
    n = len(x64)
    _, comp = connected_components(coo_matrix((np.ones(len(cc), np.int8), (cc[:, 0], cc[:, 1])), shape=(n, n)), directed=False)
    t['connected_components'] = time.perf_counter() - t0
    return t, len(np.unique(comp[core])), len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--eps', type=float, nargs='+', default=[0.005, 0.01, 0.05])
    ap.add_argument('--min-points', type=int, default=10)
    ap.add_argument('--planes', type=int, default=1000)
    ap.add_argument('--threshold', type=float, default=0.005)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--max-pairs', type=float, default=1.5e8)
    ap.add_argument('--no-host', action='store_true', help='skip the scipy and numpy runs')
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    res = {'kernels': kernel_resources('segment.hip')}
    print('kernels', json.dumps(res['kernels']), flush=True)
    if args.resources:
        return
    import torch
    from nksr_amd import cloud, ops, segment, utils
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import _grid_args
    dev = torch.device('cuda:0')
    res['device'] = torch.cuda.get_device_name(0)
    res['clocks'] = 'as found (not pinned); spread = min / max next to every median'
    x_np, _ = utils.synth_rounded_box(args.n, seed=0)
    xyz = torch.from_numpy(x_np).to(dev)
    n, m = args.n, args.min_points
    res['index_build'] = _clock(lambda: cloud.CloudIndex(xyz), 3)
    index = cloud.CloudIndex(xyz)
    tree = None
    for eps in args.eps:
        out = {}

        def fresh_grid():
            index._radius_grids.clear()
            return index._radius_grid(eps)
        out['grid'] = _clock(fresh_grid, max(3, args.reps // 3))
        g = index._radius_grid(eps)
        ga = _grid_args(g)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        full = torch.empty(n, dtype=torch.int32, device=dev)
        parent = torch.empty(n, dtype=torch.int32, device=dev)
        flags = torch.empty(n + 1, dtype=torch.int32, device=dev)
        first = torch.empty(n, dtype=torch.int32, device=dev)
        parent0, flags0 = torch.empty_like(parent), torch.empty_like(flags)          # (the unhooked forest of `init_flatten`)
        call('nksr_radius_count', ptr(g.xyz), n, *ga, None, n, eps, m, 0, None, ptr(count), stream())
        core = (count >= m).to(torch.uint8)
        r = index.cluster_dbscan(eps, m)
        label = torch.empty(n, dtype=torch.int32, device=dev)
        label[:] = r.labels[g.perm].int()                   # the labels in the grid's order: the border kernel rewrites the non-core ones
        no_pairs = torch.empty((0, 2), dtype=torch.int32, device=dev)
        out.update(_events({
            'core': lambda: call('nksr_radius_count', ptr(g.xyz), n, *ga, None, n, eps, m, 0, None, ptr(count), stream()),
            'count_uncapped': lambda: call('nksr_radius_count', ptr(g.xyz), n, *ga, None, n, eps, 0, 0, None, ptr(full), stream()),
            'components': lambda: call('nksr_dbscan_components', ptr(g.xyz), n, *ga, eps, ptr(core), ptr(parent), ptr(flags), stream()),
            'init_flatten': lambda: call('nksr_uf_components', ptr(parent0), n, ptr(core), ptr(no_pairs), 0, ptr(flags0), stream()),
            'min_caller': lambda: call('nksr_dbscan_min_caller', ptr(parent), ptr(g.perm), n, ptr(first), stream()),
            'border': lambda: call('nksr_dbscan_border', ptr(g.xyz), n, *ga, eps, ptr(core), ptr(label), stream()),
        }, args.reps))
        member = torch.nonzero(r.labels >= 0).flatten()
        sl, order = ops.sort_pairs(r.labels[member], member.to(torch.int32), end_bit=ops._bits(max(r.n_clusters, 1)))
        start = ops.sorted_runs(sl)[1]
        if r.n_clusters:
            out.update(_events({'stats_reduce': lambda: cloud.voxel_reduce(order, start[:-1], start[1:], index.xyz)}, args.reps))
        out['stats'] = _clock(lambda: segment.cluster_stats(index.xyz, r.labels, r.n_clusters), args.reps)
        out['total'] = _clock(lambda: index.cluster_dbscan(eps, m), args.reps)
        pairs = (int(full.long().sum()) - n) // 2
        info = {'n': n, 'eps': eps, 'min_points': m, 'cell': g.cell, 'points_per_cell': n / g.start.numel(), 'pairs': pairs,
                'neighbours_mean': float(full.float().mean()), 'core': int(core.sum()), 'clusters': r.n_clusters,
                'noise': int((r.labels < 0).sum()), 'largest': int(r.sizes.max()) if r.n_clusters else 0,
                'hook_over_uncapped_count': out['components']['median'] / out['count_uncapped']['median']}
        again = index.cluster_dbscan(eps, m)
        assert torch.equal(r.labels, again.labels) and torch.equal(r.centroid.view(torch.int32), again.centroid.view(torch.int32))
        if not args.no_host and pairs <= args.max_pairs:
            from scipy.spatial import cKDTree
            x64 = x_np.astype(np.float64)
            if tree is None:
                t0 = time.perf_counter()
                tree = cKDTree(x64)
                res['ckdtree_build_s'] = time.perf_counter() - t0
            sec, host_clusters, host_pairs = host_dbscan(x64, tree, eps, m)
            out['host'] = {'median': sum(sec.values()) * 1e3, 'parts_ms': {k: v * 1e3 for k, v in sec.items()}, 'note': 'one run'}
            info.update(host_clusters=host_clusters, host_pairs=host_pairs, host_over_gpu_total=sum(sec.values()) * 1e3 / out['total']['median'])
        elif not args.no_host:
            out['host'] = {'note': 'not run: %d pairs (%.0f GB as int64 index pairs)' % (pairs, pairs * 16 / 1e9)}
        res['dbscan_eps%g' % eps] = {'ms': out, 'info': info}
        print('dbscan_eps%g' % eps, json.dumps(res['dbscan_eps%g' % eps]), flush=True)
    # ---- plane RANSAC
    h, t = args.planes, args.threshold
    out = {'sample': _clock(lambda: segment.sample_planes(xyz, h, 0), args.reps)}
    planes, _ = segment.sample_planes(xyz, h, 0)
    pl = torch.from_numpy(planes).to(dev)
    counts = torch.empty(h, dtype=torch.int32, device=dev)
    ps = segment.PlanePass(xyz, t)
    best = int(np.argmax(segment.plane_scores(xyz, planes, t).cpu().numpy()))
    ps.run(planes[best])
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    out.update(_events({
        'score': lambda: call('nksr_plane_score', ptr(xyz), n, ptr(pl), h, t, ptr(counts), stream()),
        'moments': lambda: call('nksr_plane_moments', ptr(xyz), n, ps.rows.args_ptr, ps.rows.centre_ptr, t, ptr(mask), ptr(ps.rows.partials), stream()),
        'reduce': lambda: call('nksr_icp_reduce', ptr(ps.rows.partials), ps.rows.nrows, ptr(ps.rows.sums), stream()),
    }, args.reps))
    out['total'] = _clock(lambda: segment.segment_plane(xyz, t, num_iterations=h, seed=0), args.reps)
    got = counts.cpu().numpy()
    info = {'n': n, 'planes': h, 'threshold': t, 'best': best, 'best_count': int(got[best]),
            'residuals_per_s': n * h / (out['score']['median'] * 1e-3)}
    if not args.no_host:
        x64 = x_np.astype(np.float64)
        t0 = time.perf_counter()
        want = np.array([(np.abs(((p[0] * x64[:, 0] + p[1] * x64[:, 1]) + p[2] * x64[:, 2]) + p[3]) <= t).sum() for p in planes])
        sec = time.perf_counter() - t0
        out['numpy_score'] = {'median': sec * 1e3, 'note': 'one run, one core'}
        info.update(counts_equal_numpy=bool(np.array_equal(got, want)), numpy_over_gpu_score=sec * 1e3 / out['score']['median'])
    res['plane'] = {'ms': out, 'info': info}
    print('plane', json.dumps(res['plane']), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
