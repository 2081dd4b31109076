"""Per-stage times of the point-cloud preprocessing (nksr_amd/cloud.py; csrc/cloud.hip, csrc/knn_query.hip).

    python -m nksr_amd.tools.prof_cloud_ops [--sizes 1000000 10000000] [--voxel 0.1] [--reps 5] [--json OUT]

Input: ``utils.synth_scene`` (n points, 40 x 40 x 10, normals as the attribute).  HIP events, median of --reps warm runs.
  voxel downsampling   keys (nksr_point_keys), sort (radix sort of key / index pairs), runs (ops.sorted_runs: the run table), reduce
                       (nksr_voxel_reduce, xyz + 3 attribute channels), and the same with the nearest-point pass.  Next to it the
                       plain-torch formulation of the same means: key -> torch.unique(return_inverse) -> index_add_ -> divide.
                       Byte model of the reduce kernel: 12 B xyz + 4 B index + 4 C B attribute per point, (12 + 4 C + 4) B per voxel.
  neighbour search     CloudIndex build (grid + octree), then self-queries of the whole cloud: nksr_knn_query_pyramid at k = 8 / 16
                       next to nksr_knn_mean_dist_pyramid (the same traversal without the stores), and nksr_radius_count at the
                       radius that holds ~16 neighbours, with and without cap = 8.
"""
import argparse
import json

import numpy as np
import torch

from nksr_amd import cloud, ops, utils
from nksr_amd._lib import call, ptr, stream
from nksr_amd.svh import inv_w0_f32


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def downsample_stages(xyz, nrm, voxel, reps):
    n, dev = xyz.shape[0], xyz.device
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    ar = torch.arange(n, dtype=torch.int32, device=dev)
    out = {}
    out['keys'] = _time(lambda: call('nksr_point_keys', ptr(xyz), n, inv_w0_f32(voxel), ptr(keys), stream()), reps)
    out['sort'] = _time(lambda: ops.sort_pairs(keys, ar), reps)
    ks, order = ops.sort_pairs(keys, ar)

    def runs():
        s = ops.sorted_runs(ks, keys=True)[1]
        return s[:-1], s[1:]
    out['runs'] = _time(runs, reps)
    start, end = runs()
    nv = start.numel()
    out['reduce'] = _time(lambda: cloud.voxel_reduce(order, start, end, xyz, nrm), reps)
    out['reduce_nearest'] = _time(lambda: cloud.voxel_reduce(order, start, end, xyz, nrm, nearest=True), reps)
    out['total'] = out['keys'] + out['sort'] + out['runs'] + out['reduce']
    out['voxel_downsample'] = _time(lambda: cloud.voxel_downsample(xyz, voxel, normal=nrm), reps)

    def torch_path(dtype=torch.float64):
        k = torch.empty(n, dtype=torch.int64, device=dev)
        call('nksr_point_keys', ptr(xyz), n, inv_w0_f32(voxel), ptr(k), stream())
        uk, inv, cnt = torch.unique(k, return_inverse=True, return_counts=True)
        acc = torch.zeros((uk.numel(), 6), dtype=dtype, device=dev)
        acc.index_add_(0, inv, torch.cat([xyz, nrm], 1).to(dtype))
        return (acc / cnt[:, None]).float()
    out['torch'] = _time(torch_path, reps)                                     # fp64 sums like the kernel's (atomics: not repeatable)
    out['torch_fp32'] = _time(lambda: torch_path(torch.float32), reps)         # the cheaper, less accurate form
    c = nrm.shape[1]
    model_bytes = n * (12 + 4 + 4 * c) + nv * (12 + 4 * c + 4 + 8)
    info = {'points': n, 'voxels': nv, 'torch_over_kernel_path': out['torch'] / out['total'], 'reduce_model_bytes': model_bytes,
            'reduce_GBps_of_model': model_bytes / out['reduce'] / 1e6}
    m1 = cloud.voxel_reduce(order, start, end, xyz, nrm)[0]
    assert torch.allclose(m1, torch_path()[:, :3], rtol=0, atol=1e-5)
    return out, info


def search_stages(xyz, reps):
    n, dev = xyz.shape[0], xyz.device
    out = {'index_build': _time(lambda: cloud.CloudIndex(xyz), max(1, reps // 2))}
    ci = cloud.CloudIndex(xyz)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    f = torch.empty(n, dtype=torch.float32, device=dev)
    for k in (8, 16):
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
        out['knn_query_k%d' % k] = _time(lambda: call('nksr_knn_query_pyramid', ci.pyramid.struct, n, None, n, k, 0, None, 4, ptr(idx), ptr(d2),
                                                      ptr(valid), stream()), reps)
        out['knn_mean_dist_k%d' % k] = _time(lambda: call('nksr_knn_mean_dist_pyramid', ci.pyramid.struct, n, k, 4, ptr(f), ptr(valid), stream()), reps)
    call('nksr_knn_mean_dist_pyramid', ci.pyramid.struct, n, 16, 4, ptr(f), ptr(valid), stream())
    radius = float(f.median()) * 2.0                  # the mean distance to 16 neighbours is ~2/3 of the radius that holds them
    out['radius_grid_build'] = _time(lambda: (ci._radius_grids.clear(), ci._radius_grid(radius)), max(1, reps // 2))
    out['radius_count'] = _time(lambda: ci.radius_count(radius), reps)
    out['radius_count_cap8'] = _time(lambda: ci.radius_count(radius, cap=8), reps)
    info = {'radius': radius, 'mean_count': float(ci.radius_count(radius).float().mean())}
    for k in (8, 16):
        info['knn_query_k%d_Mq_per_s' % k] = n / out['knn_query_k%d' % k] / 1e3
        info['knn_mean_dist_k%d_Mq_per_s' % k] = n / out['knn_mean_dist_k%d' % k] / 1e3
    info['radius_count_Mq_per_s'] = n / out['radius_count'] / 1e3
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1_000_000, 10_000_000])
    ap.add_argument('--voxel', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {}
    for n in args.sizes:
        x, nr = utils.synth_scene(n, seed=0)
        xyz, nrm = torch.from_numpy(x).to(dev), torch.from_numpy(nr).to(dev)
        ds, ds_info = downsample_stages(xyz, nrm, args.voxel, args.reps)
        se, se_info = search_stages(xyz, args.reps)
        res[str(n)] = {'downsample_ms': ds, 'downsample': ds_info, 'search_ms': se, 'search': se_info}
        print(n, json.dumps(res[str(n)]), flush=True)
        del xyz, nrm
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
