"""Time of global registration (nksr_amd/global_register.py; csrc/fpfh.hip, csrc/global_register.hip) stage by stage.

    python -m nksr_amd.tools.prof_feature_register [--n 2000 20000 50000] [--hyp 1000 10000 100000] [--reps 9] [--no-host]
                                                   [--host-max-pairs 4e8] [--json OUT]
    python -m nksr_amd.tools.prof_feature_register --resources      (no GPU needed: compiles the two files and prints what the compiler
                                                                     reports for their kernels -- registers, spills, LDS, occupancy)

Input per size n: two samples (seeds 0 and 1) of a rounded box with a sphere and a torus (n + n / 3 + n / 3 points, analytic normals),
the second moved 140 degrees and 0.86 away.  The feature radius is 1.05 x the mean distance to the 32nd neighbour, so that it holds
about max_nn = 32 points, as a voxel-downsampled cloud at radius = 3 voxels does; the RANSAC distance is a fifth of it.  HIP events
around the launches, a host clock around what ends in a synchronise; every figure is the median of --reps warm runs with the smallest
and largest next to it; the kernels of one size are timed alternately inside one loop.

  index      cloud.CloudIndex of one cloud (host clock);  knn: CloudIndex.knn_d2(32, exclude_self) (host clock)
  spfh       nksr_spfh;  fpfh: nksr_fpfh;  feature: compute_fpfh_feature, index built (host clock)
  match      nksr_feature_match, source -> target (the key memset, k_feature_match, k_feature_match_finish)
  hypotheses global_register.ransac_hypotheses on the pairs read back: drawing, edge-length test, batched Kabsch (host clock, numpy)
  score_H    nksr_pose_score of H transforms on the matched pairs (the surviving hypotheses repeated up to H), launches of 65 536
  refit      nksr_corr_accumulate + nksr_icp_reduce
  ransac     registration_ransac_based_on_feature_matching, 100 000 draws, no mutual filter (host clock)
  host_match / host_score_1000   the same results in numpy on the host (fp32 differences in ascending j, 512 rows at a time; fp64
             residuals, one transform at a time): one run, one core; they must equal the GPU's.  host_match is left out above
             --host-max-pairs pairs of rows.
"""
import argparse
import json
import time

import numpy as np

from .prof_register import _clock, _events, kernel_resources


def shape(n, seed):
    from nksr_amd import utils
    parts = [utils.synth_rounded_box(n, seed=seed), utils.synth_sphere(n // 3, radius=0.13, seed=seed, center=(0.24, 0.14, 0.12)),
             utils.synth_torus(n // 3, R=0.12, r=0.04, seed=seed, center=(-0.15, -0.05, 0.19))]
    return np.concatenate([p[0] for p in parts]).astype(np.float32), np.concatenate([p[1] for p in parts]).astype(np.float32)


def pose():
    u, t = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.radians(140.0)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
    T[:3, 3] = [0.7, -0.4, 0.3]
    return T


def host_match(A, B, rows=512):
    idx, best = np.empty(len(A), np.int32), np.empty(len(A), np.float32)
    for lo in range(0, len(A), rows):
        a = A[lo:lo + rows]
        D = np.zeros((len(a), len(B)), np.float32)
        for j in range(A.shape[1]):
            d = a[:, j, None] - B[None, :, j]
            D += d * d
        idx[lo:lo + rows] = np.argmin(D, axis=1)
        best[lo:lo + rows] = D[np.arange(len(a)), idx[lo:lo + rows]]
    return idx, best


def host_score(src, tgt, transforms, threshold):
    s, q = src.astype(np.float64), tgt.astype(np.float64)
    out = np.empty(len(transforms), np.int32)
    for h, T in enumerate(transforms):
        p = np.stack([((T[a, 0] * s[:, 0] + T[a, 1] * s[:, 1]) + T[a, 2] * s[:, 2]) + T[a, 3] for a in range(3)], axis=1)
        e = p - q
        out[h] = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= threshold * threshold).sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[2000, 20000, 50000], help='points per cloud')
    ap.add_argument('--hyp', type=int, nargs='+', default=[1000, 10000, 100000])
    ap.add_argument('--draws', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy runs')
    ap.add_argument('--host-max-pairs', type=float, default=4e8)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    res = {'kernels': dict(kernel_resources('fpfh.hip'), **kernel_resources('global_register.hip'))}
    print('kernels', json.dumps(res['kernels']), flush=True)
    if args.resources:
        return
    import torch
    from nksr_amd import cloud, global_register as gr
    from nksr_amd._lib import call, ptr, stream
    dev = torch.device('cuda:0')
    res['device'] = torch.cuda.get_device_name(0)
    res['clocks'] = 'as found (not pinned); spread = min / max next to every median'
    T_true = pose()
    for total in args.n:
        n = total * 3 // 5                                  # n + n / 3 + n / 3 = total
        tx, tn = shape(n, 0)
        sx, sn = shape(n, 1)
        inv = np.linalg.inv(T_true)
        sx = (sx.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        sn = (sn.astype(np.float64) @ inv[:3, :3].T).astype(np.float32)
        src, src_n, tgt, tgt_n = (torch.from_numpy(a).to(dev) for a in (sx, sn, tx, tn))
        out = {'index': _clock(lambda: cloud.CloudIndex(tgt), 3)}
        si, ti = cloud.CloudIndex(src), cloud.CloudIndex(tgt)
        out['knn'] = _clock(lambda: ti.knn_d2(32, exclude_self=True), args.reps)
        radius = 1.05 * float(torch.sqrt(ti.knn_d2(32, exclude_self=True)[1][:, -1]).mean())
        distance = 0.2 * radius
        out['feature'] = _clock(lambda: ti.compute_fpfh_feature(tgt_n, radius), args.reps)
        fs, ft = si.compute_fpfh_feature(src_n, radius), ti.compute_fpfh_feature(tgt_n, radius)
        unit = (tgt_n.double() / tgt_n.double().norm(dim=1, keepdim=True)).float().contiguous()
        ns, nt = fs.data.shape[0], ft.data.shape[0]
        count, nn, mask, feat = (torch.empty_like(a) for a in (ft.spfh_count, ft.n_neighbours, ft.neighbour_mask, ft.data))
        keys = torch.empty(ns, dtype=torch.int64, device=dev)
        midx = torch.empty(ns, dtype=torch.int32, device=dev)
        md2 = torch.empty(ns, dtype=torch.float32, device=dev)
        k = ft.neighbour_idx.shape[1]
        out.update(_events({
            'spfh': lambda: call('nksr_spfh', ptr(ti.xyz), ptr(unit), nt, ptr(ft.neighbour_idx), ptr(ft.neighbour_d2), k, radius, ptr(count), ptr(nn),
                                 ptr(mask), stream()),
            'fpfh': lambda: call('nksr_fpfh', ptr(ft.spfh_count), ptr(ft.n_neighbours), ptr(ft.neighbour_mask), nt, ptr(ft.neighbour_idx),
                                 ptr(ft.neighbour_d2), k, ptr(feat), stream()),
            'match': lambda: call('nksr_feature_match', ptr(fs.data), ns, ptr(ft.data), nt, ptr(keys), ptr(midx), ptr(md2), stream()),
        }, args.reps))
        assert torch.equal(count, ft.spfh_count) and torch.equal(feat.view(torch.int32), ft.data.view(torch.int32))
        idx = midx.long()
        sp, tp = src.contiguous(), tgt[idx].contiguous()
        pairs = torch.stack([sp, tp]).cpu().numpy()
        out['hypotheses'] = _clock(lambda: gr.ransac_hypotheses(pairs[0], pairs[1], args.draws, 0.9, 0), 3)
        transforms, draw, n_drawn = gr.ransac_hypotheses(pairs[0], pairs[1], args.draws, 0.9, 0)
        info = {'points': [ns, nt], 'radius': radius, 'distance': distance, 'neighbours_mean': float(ft.n_neighbours.float().mean()),
                'draws': args.draws, 'n_drawn': n_drawn, 'n_scored': len(draw),
                'true_matches': float((((tgt[idx] - cloud.apply_transform(src, T_true)).norm(dim=1)) <= distance).float().mean())}
        if len(draw):
            for h in args.hyp:
                T = torch.from_numpy(np.resize(transforms.reshape(-1, 12), (h, 12))).to(dev)
                counts = torch.empty(h, dtype=torch.int32, device=dev)

                def score(T=T, counts=counts, h=h):
                    for lo in range(0, h, gr.SCORE_BATCH):
                        m = min(gr.SCORE_BATCH, h - lo)
                        call('nksr_pose_score', ptr(sp), ptr(tp), ns, T.data_ptr() + 96 * lo, m, distance, counts.data_ptr() + 4 * lo, stream())
                out.update(_events({'score_%d' % h: score}, args.reps))
                info['residuals_per_s_%d' % h] = ns * h / (out['score_%d' % h]['median'] * 1e-3)
            best = int(np.argmax(gr.pose_scores(sp, tp, transforms, distance).cpu().numpy()))
            t64 = pairs[1].astype(np.float64)
            centre = 0.5 * (t64.min(0) + t64.max(0))
            out.update(_events({'refit': lambda: gr.corr_sums(sp, tp, transforms[best], centre, distance)}, args.reps))
            out['ransac'] = _clock(lambda: cloud.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, distance, mutual_filter=False,
                                                                                               max_iteration=args.draws), 3)
            r = cloud.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, distance, mutual_filter=False, max_iteration=args.draws)
            Tf = r.transformation.numpy()
            dR = Tf[:3, :3] @ T_true[:3, :3].T
            info.update(best_count=r.best_count, fitness=r.fitness, pose_error_deg=float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))),
                        pose_error_translation=float(np.linalg.norm(Tf[:3, 3] - T_true[:3, 3])))
        if not args.no_host:
            if float(ns) * nt <= args.host_max_pairs:
                A, B = fs.data.cpu().numpy(), ft.data.cpu().numpy()
                t0 = time.perf_counter()
                hi, hd = host_match(A, B)
                sec = time.perf_counter() - t0
                out['host_match'] = {'median': sec * 1e3, 'note': 'one run, one core'}
                info.update(match_equals_numpy=bool(np.array_equal(hi, midx.cpu().numpy()) and np.array_equal(hd.view(np.int32), md2.cpu().numpy().view(np.int32))),
                            numpy_over_gpu_match=sec * 1e3 / out['match']['median'])
            else:
                out['host_match'] = {'note': 'not run: %d x %d rows' % (ns, nt)}
            if len(draw):
                T1k = np.resize(transforms.reshape(-1, 12), (1000, 12)).reshape(-1, 3, 4)
                t0 = time.perf_counter()
                want = host_score(pairs[0], pairs[1], T1k, distance)
                sec = time.perf_counter() - t0
                out['host_score_1000'] = {'median': sec * 1e3, 'note': 'one run, one core'}
                info['score_equals_numpy'] = bool(np.array_equal(want, gr.pose_scores(sp, tp, T1k, distance).cpu().numpy()))
        res['n%d' % total] = {'ms': out, 'info': info}
        print('n%d' % total, json.dumps(res['n%d' % total]), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
