"""Time of moving-least-squares projection (nksr_amd/mls.py; csrc/mls.hip) and of its parts.

    python -m nksr_amd.tools.prof_mls [--n 1000000] [--radius 0.005 0.01 0.05] [--reps 9] [--host-queries 2000] [--no-host] [--json OUT]
    python -m nksr_amd.tools.prof_mls --resources        (no GPU needed: compiles csrc/mls.hip and prints what the compiler reports for
                                                          its kernels -- registers, spills, scratch, LDS, occupancy)
    python -m nksr_amd.tools.prof_mls --sweep            (what the smoothing is worth to a reconstruction: ``utils.synth_sphere`` of radius
                                                          0.45 with 20 000 / 200 000 points and noise 0.006 / 0.01 / 0.02, reconstructed at
                                                          voxel_size 0.02 as it comes and through get_mls_smooth_preprocess_fn over three
                                                          radii, both orders, one and two iterations: the RMS radial error of the points and
                                                          of the mesh vertices; '<' marks a mesh closer to the sphere than the unsmoothed one)

Input: ``utils.synth_rounded_box``, n points (seed 0) with its normals, the cloud of profiles/segment.md: the three radii give 11 / 42 /
1 025 points per grid cell.  HIP events around the launches, a host clock around what ends in a synchronise; every figure is the median
of --reps warm runs with the smallest and largest next to it.  Per radius (the grid is ``CloudIndex._radius_grid(radius)``):
  grid          the PointGrid of the radius (keys, sort, cell ranges, hash): once per (index, radius)
  count         nksr_radius_count without a cap on the same grid: the same walk and coordinate loads, integers only -- the floor
  order1        nksr_mls_project, order 1, with input normals, query NULL (one walk)
  order2        the same at order 2 (two walks)
  order2_nonrm  order 2 without input normals
  project       CloudIndex.mls_project (order 2, normals) with the grid built: the launch, the gather of the normals into the grid's
                order and the scatter of the seven outputs back to the caller's (host clock)
  smooth        cloud.smooth_mls, one iteration, from the caller's tensors: CloudIndex, grid, project, the two selects (host clock)
  host          tests/mls_ref.py (numpy + cKDTree, float64, batched) on --host-queries of the points, one run, its tree build (timed
                apart: ckdtree_build_s) included; scaled to n queries (the build counted once) next to it, and the largest difference
                between its rows and the GPU's
and a model of the order-2 launch: fp64 operations per neighbour inside the radius (walk 1: 48, + 6 with normals; walk 2: 113; the
exponential counted as 20), 8 fp32 operations and 12 bytes of coordinates per candidate and walk -- a candidate is a point of the 27
cells around the query's, counted exactly from the grid's cell populations -- 24 more bytes per neighbour and walk for the fp64
re-read, all from the caches; and the compulsory traffic: 24 bytes in and 81 bytes out per query.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from .prof_register import _clock, _events, kernel_resources

FLOPS_WALK1, FLOPS_NORMALS, FLOPS_WALK2, FLOPS_CANDIDATE_FP32 = 48, 6, 113, 8
BYTES_IN, BYTES_OUT = 24, 3 * 8 + 3 * 8 + 3 * 8 + 4 + 1             # coordinates + normal; the seven outputs


def candidates_per_query(g):
    """mean number of points in the 27 cells around a point's cell, from the grid's cell populations (host side, exact)"""
    keys = g.grid.keys.cpu().numpy().astype(np.uint64)
    pop = (g.end - g.start).cpu().numpy().astype(np.int64)

    def compact(v):                                   # every third bit of a Morton key
        v = v & np.uint64(0x1249249249249249)
        for s, m in ((2, 0x10C30C30C30C30C3), (4, 0x100F00F00F00F00F), (8, 0x1F0000FF0000FF), (16, 0x1F00000000FFFF), (32, 0x1FFFFF)):
            v = (v | (v >> np.uint64(s))) & np.uint64(m)
        return v.astype(np.int64)
    c = np.stack([compact(keys >> np.uint64(a)) for a in range(3)], 1)
    c -= c.min(0)
    dim = c.max(0) + 3
    lin = ((c[:, 0] + 1) * dim[1] + (c[:, 1] + 1)) * dim[2] + (c[:, 2] + 1)
    order = np.argsort(lin)
    lin_s, pop_s = lin[order], pop[order]
    total = np.zeros(len(lin), np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = lin + (dx * dim[1] + dy) * dim[2] + dz
                j = np.clip(np.searchsorted(lin_s, want), 0, len(lin_s) - 1)
                total += np.where(lin_s[j] == want, pop_s[j], 0)
    return float((total * pop).sum() / pop.sum())


def host_rows(ref, x_np, n_np, rows, radius, order):
    """tests/mls_ref.py on the rows ``rows`` of the cloud: -> (seconds, result dict)"""
    t0 = time.perf_counter()
    r = ref.mls_project(x_np, radius, normal=n_np, query=x_np[rows], order=order)
    return time.perf_counter() - t0, r


def sweep():
    import torch
    import nksr_amd as nksr
    dev = torch.device('cuda:0')
    rec = nksr.Reconstructor(dev)

    def rms(p, r=0.45):
        return float((torch.linalg.norm(p.double(), dim=1) - r).pow(2).mean().sqrt())
    for n, seed in ((20000, 3), (200000, 0)):
        for noise in (0.006, 0.01, 0.02):
            xyz, nrm = nksr.utils.synth_sphere(n, 0.45, noise, seed=seed)
            x, nn = torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev)
            raw = rms(rec.reconstruct(x, nn, voxel_size=0.02).extract_dual_mesh(mise_iter=1).v)
            print('n %d noise %g: points %.5f, mesh as it comes %.5f' % (n, noise, rms(x), raw), flush=True)
            for h in ((0.04, 0.06, 0.1) if n == 20000 else (0.02, 0.03, 0.05)):
                for order in (1, 2):
                    for it in (1, 2):
                        fn = nksr.get_mls_smooth_preprocess_fn(h, order=order, iterations=it)
                        moved = fn(x, nn, None)[0]
                        m = rms(rec.reconstruct(x, nn, preprocess_fn=fn, voxel_size=0.02).extract_dual_mesh(mise_iter=1).v)
                        print('   h %g order %d iterations %d: points %.5f, mesh %.5f %s' % (h, order, it, rms(moved), m, '<' if m < raw else ''), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--radius', type=float, nargs='+', default=[0.005, 0.01, 0.05])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--host-queries', type=int, default=2000)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement')
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if args.sweep:
        return sweep()
    res = {'kernels': kernel_resources('mls.hip')}
    print('kernels', json.dumps(res['kernels']), flush=True)
    if args.resources:
        return
    import torch
    from nksr_amd import cloud, utils
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import _grid_args
    ref = None
    if not args.no_host:
        tests = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'tests')
        if os.path.exists(os.path.join(tests, 'mls_ref.py')):
            sys.path.insert(0, tests)
            import mls_ref as ref
    dev = torch.device('cuda:0')
    res['device'] = torch.cuda.get_device_name(0)
    res['clocks'] = 'as found (not pinned); spread = min / max next to every median'
    x_np, n_np = utils.synth_rounded_box(args.n, seed=0)
    xyz, nrm = torch.from_numpy(x_np).to(dev), torch.from_numpy(n_np).to(dev)
    n = args.n
    res['index_build'] = _clock(lambda: cloud.CloudIndex(xyz), 3)
    index = cloud.CloudIndex(xyz)
    rows = np.random.RandomState(0).choice(n, min(args.host_queries, n), replace=False)
    for radius in args.radius:
        out = {}

        def fresh_grid():
            index._radius_grids.clear()
            return index._radius_grid(radius)
        out['grid'] = _clock(fresh_grid, max(3, args.reps // 3))
        g = index._radius_grid(radius)
        ga = _grid_args(g)
        ns = nrm[g.perm].contiguous()
        count = torch.empty(n, dtype=torch.int32, device=dev)
        pos, no = torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev)
        hc, kc, var = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        cnt, used = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
        h32 = float(np.float32(radius))

        def launch(order, normals):
            call('nksr_mls_project', ptr(g.xyz), n, *ga, ptr(ns) if normals else None, None, n, h32, 0.5 * h32, order, 3 if order == 1 else 8,
                 ptr(pos), ptr(no), ptr(hc), ptr(kc), ptr(var), ptr(cnt), ptr(used), stream())
        out.update(_events({
            'count': lambda: call('nksr_radius_count', ptr(g.xyz), n, *ga, None, n, radius, 0, 0, None, ptr(count), stream()),
            'order1': lambda: launch(1, True),
            'order2': lambda: launch(2, True),
            'order2_nonrm': lambda: launch(2, False),
        }, args.reps))
        out['project'] = _clock(lambda: index.mls_project(radius, normal=nrm), args.reps)
        out['smooth'] = _clock(lambda: cloud.smooth_mls(xyz, radius, normal=nrm), max(3, args.reps // 3))
        r = index.mls_project(radius, normal=nrm)
        again = index.mls_project(radius, normal=nrm)
        assert torch.equal(r.position.view(torch.int64), again.position.view(torch.int64)) and torch.equal(r.count, count[torch.argsort(g.perm)])
        nb, cand = float(r.count.double().mean()), candidates_per_query(g)
        f64 = n * nb * (FLOPS_WALK1 + FLOPS_NORMALS + FLOPS_WALK2)
        sec = out['order2']['median'] * 1e-3
        info = {'n': n, 'radius': radius, 'cell': g.cell, 'points_per_cell': n / g.start.numel(), 'neighbours_mean': nb,
                'neighbours_max': int(r.count.max()), 'candidates_mean': cand, 'order_used': torch.bincount(r.order_used.long(), minlength=3).tolist(),
                'order2_over_count': out['order2']['median'] / out['count']['median'],
                'model': {'fp64_flop': f64, 'fp64_tflops_achieved': f64 / sec / 1e12,
                          'fp32_flop': 2 * n * cand * FLOPS_CANDIDATE_FP32, 'cache_bytes': 2 * n * cand * 12 + 2 * n * nb * 24,
                          'cache_GBps_achieved': (2 * n * cand * 12 + 2 * n * nb * 24) / sec / 1e9,
                          'compulsory_bytes': n * (BYTES_IN + BYTES_OUT), 'compulsory_GBps_achieved': n * (BYTES_IN + BYTES_OUT) / sec / 1e9,
                          'ns_per_neighbour': sec * 1e9 / (n * nb)}}
        if ref is not None:
            from scipy.spatial import cKDTree
            if 'ckdtree_build_s' not in res:
                t0 = time.perf_counter()
                cKDTree(x_np.astype(np.float64))
                res['ckdtree_build_s'] = time.perf_counter() - t0
            host = {}
            for order in (1, 2):
                s, hr = host_rows(ref, x_np, n_np, rows, radius, order)
                build = min(res['ckdtree_build_s'], s)
                host['order%d' % order] = {'median': s * 1e3, 'queries': len(rows), 'scaled_to_n_ms': ((s - build) * n / len(rows) + build) * 1e3,
                                           'note': 'one run, tree build included'}
            rr = torch.from_numpy(rows).to(dev)
            # a pair within fp32 rounding of the radius is a neighbour for one side only: those rows are counted and compared apart
            same = hr['count'] == r.count[rr].cpu().numpy()
            dpos = np.abs(hr['position'] - r.position[rr].cpu().numpy()).max(1) / h32
            dnrm = np.nan_to_num(np.abs(hr['normal'] - r.normal[rr].cpu().numpy()).max(1))
            info.update(host_over_gpu_order2=host['order2']['scaled_to_n_ms'] / out['order2']['median'],
                        host_rows=len(rows), host_rows_other_count=int((~same).sum()),
                        host_rows_order_used_equal=bool(np.array_equal(hr['order_used'], r.order_used[rr].cpu().numpy())),
                        host_rows_max_position_diff_over_h=float(dpos[same].max()), host_rows_max_normal_diff=float(dnrm[same].max()),
                        other_count_rows_max_position_diff_over_h=float(dpos[~same].max()) if (~same).any() else 0.0,
                        host_rows_max_cond=float(np.nanmax(hr['cond'])))
            out['host'] = host
        res['mls_radius%g' % radius] = {'ms': out, 'info': info}
        print('mls_radius%g' % radius, json.dumps(res['mls_radius%g' % radius]), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
