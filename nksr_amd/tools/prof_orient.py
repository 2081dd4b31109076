"""Per-stage times of the sensor-free normal orientation (nksr_amd/orient.py; csrc/orient.hip).

    python -m nksr_amd.tools.prof_orient [--k 16] [--knn 64] [--reps 3] [--json OUT] [--md OUT] [--sphere 1000000] [--scene 10000000]

Inputs: ``utils.synth_sphere`` and ``utils.synth_scene``, the true normals with every sign flipped at random.  HIP events around every
stage (a synchronisation per stage, so the sum is an upper bound of the unprofiled call, which is timed next to it); median of --reps
warm runs.  Stages: kNN (``CloudIndex.knn(k, exclude_self=True)``, the index build apart), then per Boruvka round propose / hook / jump
/ relabel summed over the rounds, and seeds (seed + apply).  Per round: components at its start, points still active (not yet
surrounded by their own component) and links made.  Yardstick: ``normals.estimate_normals_knn`` on the same cloud -- kNN-PCA plus the
flip towards a sensor -- which is what a user with sensor positions pays today; next to it ``cloud.estimate_normals`` (kNN-PCA plus
this orientation)."""
import argparse
import json

import numpy as np
import torch

from nksr_amd import cloud, normals, orient, utils

STAGES = ('knn', 'propose', 'hook', 'jump', 'relabel', 'seeds')


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


def profile(xyz, nrm, k, knn, reps):
    n = xyz.shape[0]
    sign = torch.where(torch.rand(n, device=xyz.device, generator=torch.Generator(xyz.device).manual_seed(3)) < 0.5, -1.0, 1.0)
    given = (nrm * sign[:, None]).contiguous()
    out = {'points': n, 'k': k, 'index_build_ms': _time(lambda: cloud.CloudIndex(xyz), max(1, reps // 2))}
    index = cloud.CloudIndex(xyz)
    runs = []
    for _ in range(reps + 1):                      # the first run warms up
        stats = {}
        res = orient._orient_on_index(index, given, k, '+z', None, stats=stats)
        runs.append(stats)
    runs = runs[1:]
    out['stage_ms'] = {s: float(np.median([r.get(s, 0.0) for r in runs])) for s in STAGES}
    out['stages_total_ms'] = sum(out['stage_ms'].values())
    out['rounds'] = runs[-1]['rounds']
    out['components'] = res.n_components
    out['agreement_with_truth'] = float(((res.normal * nrm).sum(1) > 0).float().mean())
    out['orient_normals_ms'] = _time(lambda: index.orient_normals(given, k=k), reps)                   # unprofiled: kNN + rounds + seeds
    out['estimate_normals_ms'] = _time(lambda: cloud.estimate_normals(xyz, knn=knn, orient_k=k), reps)
    sensor = torch.zeros_like(xyz)
    sensor[:, 2] = 50.0
    out['estimate_normals_knn_sensor_ms'] = _time(lambda: normals.estimate_normals_knn(xyz, None, sensor, knn, 85.0), reps)
    return out


def table(results):
    lines = ['| cloud | points | index build | ' + ' | '.join(STAGES) + ' | stages total | `orient_normals` | `estimate_normals` | '
             '`estimate_normals_knn` (sensor) | rounds | components | agreement |', '|' + '---|' * (len(STAGES) + 10)]
    for name, r in results.items():
        lines.append('| %s | %d | %.2f | %s | %.2f | %.2f | %.2f | %.2f | %d | %d | %.4f |' % (
            name, r['points'], r['index_build_ms'], ' | '.join('%.2f' % r['stage_ms'][s] for s in STAGES), r['stages_total_ms'],
            r['orient_normals_ms'], r['estimate_normals_ms'], r['estimate_normals_knn_sensor_ms'], len(r['rounds']), r['components'],
            r['agreement_with_truth']))
    lines.append('')
    lines.append('Times in ms.  Per round (components at its start / points still active / links made):')
    for name, r in results.items():
        lines.append('')
        lines.append('* %s: ' % name + ', '.join('%d / %d / %d' % (q['components'], q['active_points'], q['links']) for q in r['rounds']))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sphere', type=int, default=1_000_000)
    ap.add_argument('--scene', type=int, default=10_000_000)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--knn', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {}
    for name, make, n in (('synth_sphere', lambda m: utils.synth_sphere(m, 0.45, 0.0, 0), args.sphere),
                          ('synth_scene', lambda m: utils.synth_scene(m, seed=0), args.scene)):
        if n <= 0:
            continue
        x, nr = make(n)
        xyz, nrm = torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(nr.astype(np.float32)).to(dev)
        res[name] = profile(xyz, nrm, args.k, args.knn, args.reps)
        print(name, json.dumps(res[name]), flush=True)
        del xyz, nrm
        torch.cuda.empty_cache()
    md = table(res)
    print(md)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(md)


if __name__ == '__main__':
    main()
