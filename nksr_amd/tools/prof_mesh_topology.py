"""Per-stage times of the GPU mesh topology (nksr_amd/mesh_topology.py, csrc/meshtopo.hip).

    python -m nksr_amd.tools.prof_mesh_topology [--scene] [--json OUT] [--reps 5] [--no-host]

Cases:
  configs2   the configs[2] mesh: the 1 M-point synth_scene (detail_level 1.0, extract_dual_mesh(mise_iter=1)), ~2.3 M triangles
  scene_4m   with --scene: the 4 M-point scene of tools/stress_4m (80 x 80 x 10, 32 objects)
Stages (HIP events, median of --reps warm runs; the read-backs of E and of the number of components are inside their stage): keys,
sort, runs (heads, scan, edge table, classes), hook + flatten with the labels for both connectivities, statistics (counts, boxes,
areas) for both, and the compaction that drops every component under 1 % of the largest one's area.  'host_ms' is the numpy half-edge
np.unique plus scipy.sparse.csgraph.connected_components on the vertex graph of the same mesh, with the copy to the host before it.
"""
import argparse
import json
import time

import numpy as np
import torch

from nksr_amd import mesh_topology as mt


def stages(v, f):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
    nv = v.shape[0]
    ev[0].record()
    keys, ids, valid, ref = mt.halfedge_keys(f, nv)
    ev[1].record()
    ks, ids_sorted = mt.sort_halfedges(keys, ids, nv)
    ev[2].record()
    t = mt.MeshTopology.from_device(v, f, (valid, ref, ks, ids_sorted, mt.edge_runs(f, nv, ks, ids_sorted, ref)))
    ev[3].record()
    ce = t.labels('edge')
    ev[4].record()
    cv = t.labels('vertex')
    ev[5].record()
    t.component_stats(ce)
    ev[6].record()
    t.component_stats(cv)
    ev[7].record()
    keep = ce.face_mask(ce.select(min_area_ratio=0.01)).to(torch.uint8)
    v2, f2, _, _ = mt.compact_mesh(v, f, keep)
    ev[8].record()
    torch.cuda.synchronize()
    names = ['keys', 'sort', 'runs', 'components_edge', 'components_vertex', 'stats_edge', 'stats_vertex', 'compaction']
    out = {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(names)}
    info = {'edges': t.num_edges, 'boundary_edges': t.boundary_edges, 'nonmanifold_edges': t.nonmanifold_edges,
            'components_edge': ce.n, 'components_vertex': cv.n, 'faces_kept': int(f2.shape[0])}
    return out, info


def host_path(mesh):
    """The same answers on the host: copy, half-edge np.unique, connected_components of the vertex graph (seconds per step)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = mesh.f.cpu().numpy().astype(np.int64)
    nv = int(mesh.v.shape[0])
    t1 = time.perf_counter()
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    uk, cnt = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_counts=True)
    t2 = time.perf_counter()
    g = coo_matrix((np.ones(len(uk), np.int8), (uk >> 32, uk & 0xFFFFFFFF)), shape=(nv, nv))
    n = connected_components(g, directed=False)[0]
    t3 = time.perf_counter()
    return {'copy': (t1 - t0) * 1e3, 'unique': (t2 - t1) * 1e3, 'connected_components': (t3 - t2) * 1e3, 'total': (t3 - t0) * 1e3}, \
        {'edges': len(uk), 'boundary_edges': int((cnt == 1).sum()), 'components_vertex': int(n)}


def case_mesh(dev, n, extent, n_objects):
    import nksr_amd
    from nksr_amd import utils
    xyz, nrm = utils.synth_scene(n, seed=0, extent=extent, n_objects=n_objects)
    rec = nksr_amd.Reconstructor(dev)
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=1.0)
    return fld.extract_dual_mesh(mise_iter=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scene', action='store_true', help='also the 4 M-point scene mesh')
    ap.add_argument('--no-host', action='store_true', help='skip the numpy / scipy timing')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cases = [('configs2', (1_000_000, (40.0, 40.0, 10.0), 8))]
    if args.scene:
        cases.append(('scene_4m', (4_000_000, (80.0, 80.0, 10.0), 32)))
    out = {}
    for name, spec in cases:
        mesh = case_mesh(dev, *spec)
        v, f = mesh.v.float().contiguous(), mesh.f.contiguous()
        stages(v, f)                                                    # warm-up
        runs = [stages(v, f) for _ in range(args.reps)]
        rec = {'vertices': int(v.shape[0]), 'faces': int(f.shape[0]), **runs[0][1],
               'gpu_ms': {k: float(np.median([r[0][k] for r in runs])) for k in runs[0][0]}}
        rec['gpu_ms']['total'] = sum(rec['gpu_ms'].values())
        if not args.no_host:
            rec['host_ms'], host_info = host_path(mesh)
            assert all(rec[k] == x for k, x in host_info.items()), (host_info, rec)
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
        del mesh, v, f
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
