"""Per-stage times of the GPU mesh queries (nksr_amd/mesh_query.py, csrc/meshquery.hip).

    python -m nksr_amd.tools.prof_mesh_query [--json OUT] [--reps 5]

Two cases:
  configs1   the configs[1] recipe mesh (3 000-point sphere, preset snet-n3k-wnormal) with 1e5 ONet-style queries (half uniform in the
             box padded by 0.1, half within N(0, 0.01) of the surface)
  scene_1m   the 1 M-point synth_scene mesh (detail_level 1.0, extract_dual_mesh(mise_iter=1)) with 1e6 queries alike
Stages (HIP events, median of --reps warm runs): the build (box + codes, sort, nodes, refit with the depth read back), the queries'
Morton order, occupancy at rays 1 and 3 and the distance, each on the sorted queries; 'occupancy3_unsorted' is the rays = 3 pass in
the given query order, the measurement behind sorting them.
"""
import argparse
import json

import numpy as np
import torch

from nksr_amd import mesh_input, mesh_query


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def stages(v32, f, q32):
    mq = mesh_query
    ev = _events(11)
    ev[0].record()
    lo, hi, _ = mq.bbox_center(v32)
    box = torch.cat([lo, hi]).contiguous()
    bvh = mq.Bvh(f.shape[0], box, v32.device)
    codes, index = mq.morton(v32, box, f, v32.shape[0])
    ev[1].record()
    ks, order = mq.sort_codes(codes, index)
    ev[2].record()
    parent = mq.build_nodes(bvh, ks)
    ev[3].record()
    mq.refit(bvh, v32, f, order, parent)
    mq.finish(bvh)
    ev[4].record()
    q = mq.MeshQuery.from_bvh(bvh, np.zeros(3))
    qc, qi = mq.morton(q32, box)
    qorder = mq.sort_codes(qc, qi)[1]
    ev[5].record()
    q._occupancy(q32, qorder, 1)
    ev[6].record()
    q._occupancy(q32, qorder, 3)
    ev[7].record()
    q._closest(q32, qorder)
    ev[8].record()
    q._occupancy(q32, None, 3)
    ev[9].record()
    q._closest(q32, None)
    ev[10].record()
    torch.cuda.synchronize()
    names = ['build_codes', 'build_sort', 'build_nodes', 'build_refit', 'query_order', 'occupancy1', 'occupancy3', 'distance',
             'occupancy3_unsorted', 'distance_unsorted']
    out = {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(names)}
    return out, bvh.depth


def onet_queries(v, n, seed=0):
    rs = np.random.RandomState(seed)
    v = np.asarray(v, np.float64)
    lo, hi = v.min(0) - 0.1 * (v.max(0) - v.min(0)), v.max(0) + 0.1 * (v.max(0) - v.min(0))
    uni = rs.uniform(lo, hi, (n // 2, 3))
    near = v[rs.randint(0, len(v), n - n // 2)] + rs.normal(0, 0.01 * np.linalg.norm(hi - lo) / np.sqrt(3), (n - n // 2, 3))
    return np.concatenate([uni, near])


def case_configs1(dev):
    import nksr
    from nksr_amd import utils
    xyz, nrm = utils.synth_sphere(3000, 0.45, 0.005, 0)
    rec = nksr.Reconstructor(dev, config='snet-n3k-wnormal')
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=None)
    return fld.extract_dual_mesh(mise_iter=1), int(1e5)


def case_scene_1m(dev):
    import nksr_amd
    from nksr_amd import utils
    xyz, nrm = utils.synth_scene(1_000_000, seed=0)
    rec = nksr_amd.Reconstructor(dev)
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=1.0)
    return fld.extract_dual_mesh(mise_iter=1), int(1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    for name, make in (('configs1', case_configs1), ('scene_1m', case_scene_1m)):
        mesh, n = make(dev)
        vn = mesh.v.cpu().numpy()
        centre = mesh_input.bbox_centre(vn)
        v32 = mesh_input.recentre(vn, centre, dev, 'v')
        f = mesh_input.faces(mesh.f, v32.shape[0], dev, cast_float=True, check_range=True)
        q32 = mesh_input.recentre(onet_queries(vn, n), centre, dev, 'q')
        stages(v32, f, q32)                                             # warm-up
        runs = []
        for _ in range(args.reps):
            r, depth = stages(v32, f, q32)
            runs.append(r)
        rec = {'faces': int(f.shape[0]), 'queries': n, 'depth': depth,
               'gpu_ms': {k: float(np.median([r[k] for r in runs])) for k in runs[0]}}
        rec['gpu_ms']['build_total'] = sum(rec['gpu_ms'][k] for k in ('build_codes', 'build_sort', 'build_nodes', 'build_refit'))
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
        del mesh
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
