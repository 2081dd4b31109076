"""Per-stage times of the GPU MeshEvaluator (nksr_amd/metrics.py) beside a CPU evaluation of the same mesh.

    python -m nksr_amd.tools.prof_metrics [--json OUT] [--reps 5]

Two cases, the reference's two sample counts (models/nksr_net.py:298-310):
  configs1   the configs[1] recipe (3 000-point sphere, preset snet-n3k-wnormal) at 5e5 samples, against 2e5 analytic points
  scene_1m   the 1 M-point synth_scene mesh (detail_level 1.0, extract_dual_mesh(mise_iter=1)) at 5e6 samples, against its input
GPU stages (HIP events, median of --reps warm runs): face areas + CDF, sampling, the two pyramids (samples, target), the two 1-NN
passes (target -> samples, samples -> target) and the reduce; 'eval_mesh' is one whole call, host work included.  The CPU column is
the same evaluation with numpy sampling and scipy cKDTree queries on 16 workers (the method of the test oracle), one run.
"""
import argparse
import json
import time

import numpy as np
import torch

from nksr_amd import mesh_input, metrics


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def gpu_stages(mesh, gt, gtn, n, dev):
    centre = mesh_input.bbox_centre(gt)
    v32 = mesh_input.recentre(mesh.v, centre, dev, 'v')
    f = mesh_input.faces(mesh.f, v32.shape[0], dev, cast_float=True, check_range=True)
    t = mesh_input.recentre(gt, centre, dev, 'gt')
    tn = mesh_input.normals32(gtn, t.shape[0], dev, 'gtn')
    ev = _events(8)
    ev[0].record()
    fn, cdf = metrics.face_cdf(v32, f)
    ev[1].record()
    p, pn, _ = metrics.sample_from_cdf(v32, f, fn, cdf, n, 0)
    ev[2].record()
    pred = metrics.Cloud(p, pn)
    ev[3].record()
    tgt = metrics.Cloud(t, tn)
    ev[4].record()
    comp = pred.nearest(tgt.xyz, tgt.normal, sums=False, dist=torch.empty(tgt.n, device=dev))
    ev[5].record()
    acc = tgt.nearest(pred.xyz, pred.normal, sums=False, dist=torch.empty(pred.n, device=dev))
    ev[6].record()
    s = pred.nearest(tgt.xyz, tgt.normal)               # the same pass with its partials, and their reduce
    ev[7].record()
    torch.cuda.synchronize()
    del comp, acc, s
    names = ['areas_cdf', 'sample', 'pyramid_samples', 'pyramid_target', 'nn_target_to_samples', 'nn_samples_to_target', 'nn_with_partials_and_reduce']
    return {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(names)}


def cpu_eval(v, f, gt, gtn, n, workers=16):
    """numpy area-weighted sampling + cKDTree(workers=16) nearest neighbours, the essential metrics (seconds, dict)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cr = np.cross(b - a, c - a)
    area = np.linalg.norm(cr, axis=1)
    rs = np.random.RandomState(0)
    j = rs.choice(len(f), size=n, p=area / area.sum())
    r1, r2 = np.sqrt(rs.rand(n)), rs.rand(n)
    p = (1 - r1)[:, None] * a[j] + (r1 * (1 - r2))[:, None] * b[j] + (r1 * r2)[:, None] * c[j]
    pn = cr[j] / np.maximum(area[j], 1e-30)[:, None]
    gt, gtn = np.asarray(gt, np.float64), np.asarray(gtn, np.float64)
    gtn = gtn / np.maximum(np.linalg.norm(gtn, axis=1, keepdims=True), 1e-30)
    dc, ic = cKDTree(p).query(gt, workers=workers)
    da, ia = cKDTree(gt).query(p, workers=workers)
    rec, prec = (dc <= 0.01).mean(), (da <= 0.01).mean()
    out = {'chamfer-L1': 0.5 * (dc.mean() + da.mean()), 'f-score': 2 * prec * rec / max(prec + rec, 1e-30),
           'normals': 0.5 * (np.abs((pn[ic] * gtn).sum(1)).mean() + np.abs((gtn[ia] * pn).sum(1)).mean())}
    return time.perf_counter() - t0, {k: float(x) for k, x in out.items()}


def case_configs1(dev):
    import nksr
    from nksr_amd import utils
    xyz, nrm = utils.synth_sphere(3000, 0.45, 0.005, 0)
    rec = nksr.Reconstructor(dev, config='snet-n3k-wnormal')
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=None)
    gt, gtn = utils.synth_sphere(200000, 0.45, 0.0, 12345)
    return fld.extract_dual_mesh(mise_iter=1), gt, gtn, int(5e5)


def case_scene_1m(dev):
    import nksr_amd
    from nksr_amd import utils
    xyz, nrm = utils.synth_scene(1_000_000, seed=0)
    rec = nksr_amd.Reconstructor(dev)
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=1.0)
    return fld.extract_dual_mesh(mise_iter=1), xyz, nrm, int(5e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    for name, make in (('configs1', case_configs1), ('scene_1m', case_scene_1m)):
        mesh, gt, gtn, n = make(dev)
        ev = metrics.MeshEvaluator(n, metrics.MeshEvaluator.ESSENTIAL_METRICS, dev)
        ev.eval_mesh(mesh, gt, gtn)
        gpu_stages(mesh, gt, gtn, n, dev)                    # warm-up
        runs, walls = [], []
        for _ in range(args.reps):
            runs.append(gpu_stages(mesh, gt, gtn, n, dev))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = ev.eval_mesh(mesh, gt, gtn)
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        rec = {'faces': int(mesh.f.shape[0]), 'samples': n, 'target_points': int(len(gt)),
               'gpu_ms': {k: float(np.median([r[k] for r in runs])) for k in runs[0]}, 'eval_mesh_ms': float(np.median(walls)), 'gpu_metrics': m}
        if not args.no_cpu:
            s, cm = cpu_eval(mesh.v.cpu().numpy(), mesh.f.cpu().numpy(), gt, gtn, n)
            rec['cpu_ckdtree16_ms'] = 1e3 * s
            rec['cpu_metrics'] = cm
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
        del mesh
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
