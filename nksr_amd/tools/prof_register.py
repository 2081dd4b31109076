"""Time of one ICP pass (nksr_amd/register.py; csrc/register.hip) and of its parts.

    python -m nksr_amd.tools.prof_register [--n 1000000] [--radii 0.01 0.05] [--reps 9] [--no-host] [--json OUT]
    python -m nksr_amd.tools.prof_register --resources          (no GPU needed: compiles csrc/register.hip and prints what the compiler
                                                                 reports for its kernels -- registers, spills, LDS, occupancy)

Input: ``utils.synth_rounded_box``, n target points (seed 0) and n source points (seed 1) moved by the inverse of a pose whose
displacement is about a third of the radius, so that the pass at identity finds nearly every correspondence.  HIP events around the
launches, a host clock around what ends in the read of the sums; every figure is the median of --reps warm runs with the smallest and
largest next to it.  Per radius and method:
  accumulate_sorted / accumulate_caller   nksr_icp_accumulate with the source sorted by its cell key at the initial pose, and in the
                                          caller's (random) order -- alternated inside one loop, so that both see the same clocks
  reduce                                  nksr_icp_reduce over the per-workgroup rows
  host_step                               the 256-byte read of the sums + kabsch_step / plane_step (fp64 numpy)
  pass                                    IcpPass.run: pose upload, both kernels, the read
  sort_source                             what the sorted order costs once per icp call (keys, radix sort, gather)
  ckdtree_pass                            the same pass on the host: scipy cKDTree query (16 workers) + the fp64 sums in numpy
                                          (tree build apart)
"""
import argparse
import json
import os
import re
import subprocess
import time

import numpy as np


def kernel_resources(source='register.hip'):
    """{kernel: {VGPRs, VGPRs Spill, SGPRs Spill, ScratchSize, Occupancy, LDS Size}} as hipcc reports them for csrc/<source>"""
    from nksr_amd import build
    cmd = [build.HIPCC] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c',
                                         os.path.join(build.CSRC, source), '-o', os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed:\n%s' % r.stderr)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|'
                      r'LDS Size \[bytes/block\]):\s+(\S+)', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = m.group(2)
            mm = re.match(r'_ZL?(\d+)', name)                 # Itanium mangling: length-prefixed name, ILi<k>E / ILb<k>E = template argument k
            if mm:
                rest = name[mm.end():]
                n = int(mm.group(1))
                t = re.match(r'IL[ib](\d+)E', rest[n:])
                name = rest[:n] + ('<%s>' % t.group(1) if t else '')
            out[name] = {}
        elif name:
            out[name][m.group(1).split(' [')[0]] = int(m.group(2))
    return out


def _stats(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms))}


def _events(fns, reps):
    """the callables of ``fns`` timed alternately: {name: stats in ms}"""
    import torch
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: _stats(v) for k, v in ms.items()}


def _clock(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return _stats(ms)


def host_pass(tree, t64, n64, source, radius, method, centre):
    """one pass at identity on the host: -> (seconds, sums)"""
    t0 = time.perf_counter()
    p = source.astype(np.float64)
    d, i = tree.query(p, k=1, distance_upper_bound=radius, workers=min(16, os.cpu_count() or 1))
    m = np.isfinite(d)
    q, pp = t64[i[m]], p[m] - centre
    dd = p[m] - q
    if method == 'point':
        qq = q - centre
        s = np.concatenate([[m.sum(), (dd * dd).sum()], pp.sum(0), qq.sum(0), (pp.T @ qq).ravel()])
    else:
        nn = n64[i[m]]
        J = np.concatenate([np.cross(pp, nn), nn], axis=1)
        r = np.einsum('ij,ij->i', nn, dd)
        s = np.concatenate([[m.sum(), (dd * dd).sum()], (J.T @ J)[np.triu_indices(6)], J.T @ r, [r @ r]])
    return time.perf_counter() - t0, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--radii', type=float, nargs='+', default=[0.01, 0.05])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--no-host', action='store_true', help='skip the cKDTree pass')
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    res = {'kernels': kernel_resources()}
    print('kernels', json.dumps(res['kernels']), flush=True)
    if args.resources:
        return
    import torch
    from nksr_amd import cloud, register, utils
    from nksr_amd._lib import call, ptr, stream
    from nksr_amd.neighbours import _grid_args
    dev = torch.device('cuda:0')
    res['device'] = torch.cuda.get_device_name(0)
    res['clocks'] = 'as found (not pinned); spread = min / max next to every median'
    t_np, n_np = utils.synth_rounded_box(args.n, seed=0)
    s_np, _ = utils.synth_rounded_box(args.n, seed=1)
    target, normal = torch.from_numpy(t_np).to(dev), torch.from_numpy(n_np).to(dev)
    index = cloud.CloudIndex(target)
    tree = None
    for radius in args.radii:
        w = radius / 3.0
        pose = np.eye(4)
        pose[:3, :3] = register.rodrigues(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0) * w)        # |w| rad: ~w / 2 at the surface
        pose[:3, 3] = np.array([0.6, -0.5, 0.3]) * w
        source = register.apply_transform(torch.from_numpy(s_np).to(dev), np.linalg.inv(pose))
        for method in ('point', 'plane'):
            nrm = normal if method == 'plane' else None
            T = np.eye(4)
            key = 'r%g_%s' % (radius, method)
            out = {}
            out['sort_source'] = _clock(lambda: register.IcpPass(index, source, radius, method, nrm, T, sort_source=True), max(3, args.reps // 3))
            ps = {True: register.IcpPass(index, source, radius, method, nrm, T, sort_source=True),
                  False: register.IcpPass(index, source, radius, method, nrm, T, sort_source=False)}
            out['sort_source']['note'] = 'IcpPass set-up with the sort; without it: %.3f ms' % _clock(
                lambda: register.IcpPass(index, source, radius, method, nrm, T, sort_source=False), max(3, args.reps // 3))['median']
            g = ps[True].grid

            def acc(p):
                call('nksr_icp_accumulate', ptr(g.xyz), index.n, *_grid_args(g), ptr(g.perm), ptr(p.normal), ptr(p.source), p.n,
                     p.rows.args_ptr, p.rows.centre_ptr, radius, p.method, ptr(p.corr), ptr(p.rows.partials), stream())
            for p in ps.values():
                p.run(T)
            rows = ps[True].rows
            ev = _events({'accumulate_sorted': lambda: acc(ps[True]), 'accumulate_caller': lambda: acc(ps[False]),
                          'reduce': lambda: call('nksr_icp_reduce', ptr(rows.partials), rows.nrows, ptr(rows.sums), stream())},
                         args.reps)
            out.update(ev)
            step = register.STEPS[method]
            out['host_step'] = _clock(lambda: step(rows.sums.cpu().numpy(), ps[True].centre), args.reps)
            out['pass'] = _clock(lambda: ps[True].run(T), args.reps)
            sums = ps[True].run(T)
            info = {'n_source': ps[True].n, 'n_target': index.n, 'cell': g.cell, 'fitness': float(sums[register.COUNT]) / ps[True].n,
                    'points_per_cell': index.n / g.start.numel(), 'sorted_over_caller': out['accumulate_sorted']['median'] / out['accumulate_caller']['median']}
            assert torch.equal(ps[True].correspondences(), ps[False].correspondences())
            if not args.no_host:
                from scipy.spatial import cKDTree
                t64, n64 = t_np.astype(np.float64), n_np.astype(np.float64)
                if tree is None:
                    t0 = time.perf_counter()
                    tree = cKDTree(t64)
                    res['ckdtree_build_s'] = time.perf_counter() - t0
                sec, hs = host_pass(tree, t64, n64, source.cpu().numpy(), radius, method, ps[True].centre)
                out['ckdtree_pass'] = {'median': sec * 1e3, 'min': sec * 1e3, 'max': sec * 1e3, 'note': 'one run'}
                info['host_over_gpu_pass'] = sec * 1e3 / out['pass']['median']
                info['count_gpu_minus_host'] = float(sums[register.COUNT] - hs[0])
            res[key] = {'ms': out, 'info': info}
            print(key, json.dumps(res[key]), flush=True)
            del ps
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
