"""Per-stage times of the GPU mesh geometry (nksr_amd/mesh_geometry.py, csrc/meshgeom.hip).

    python -m nksr_amd.tools.prof_mesh_geometry [--json OUT] [--reps 5] [--no-host]

Case: the configs[2] mesh of tools/prof_mesh_topology (1 M-point synth_scene, detail_level 1.0, extract_dual_mesh(mise_iter=1)),
~2.3 M triangles.  Stages (HIP events, median of --reps warm runs, the topology's edge table excluded: it exists already): adjacency
(directed keys, sort, row starts + unpack + vertex kinds), corner incidence (keys, sort, row starts), the face pass, normals (the
corner gather), curvature (edge weights + the adjacency gather), and ONE smoothing step (20 queued Taubin steps over 20, boundary
'free': every referenced vertex gathers its whole row, which is what the byte model charges).  The byte model of the step: per vertex
one 24 B read and one 24 B write (the row start and the kind on top: 5 B), per directed entry a 4 B index and one 24 B position
gather.  'host_ms' is the same work in numpy / scipy on the host (sparse adjacency from the faces, np.add.at normals,
one sparse-product step), with the copy to the host before it.
"""
import argparse
import json
import time

import numpy as np
import torch

from nksr_amd import mesh_geometry as mg
from nksr_amd._lib import GEOM_FREE, call, ptr, stream
from nksr_amd.mesh_topology import MeshTopology
from nksr_amd.tools.prof_mesh_topology import case_mesh

STEPS = 20


def stages(t):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    ev[0].record()
    g = mg.MeshGeometry.from_topology(t)
    ev[1].record()
    g.corners()
    ev[2].record()
    g.faces()
    ev[3].record()
    g.vertex_normals()
    ev[4].record()
    g.mean_curvature()
    xa = g.x.to(torch.float64)
    xb = torch.empty_like(xa)
    ev[5].record()
    call('nksr_geom_smooth', ptr(xa), ptr(xb), g.n_vertices, ptr(g.neighbour_start), ptr(g.neighbours), t.edges.shape[0], ptr(g.neighbour_class),
         ptr(g.vertex_kind), None, GEOM_FREE, STEPS, 0.5, -0.53, stream())
    ev[6].record()
    torch.cuda.synchronize()
    names = ['adjacency', 'corner_incidence', 'face_pass', 'normals', 'curvature', 'smooth_step']
    out = {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(names)}
    out['smooth_step'] /= STEPS
    return out, g


def step_bytes(nv, n_directed):
    """Bytes the byte model charges one smoothing step."""
    return nv * (24 + 24 + 4 + 1) + n_directed * (4 + 24)


def host_path(mesh):
    """The same results on the host (milliseconds per step)."""
    from scipy.sparse import coo_matrix
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, f = mesh.v.cpu().numpy().astype(np.float64), mesh.f.cpu().numpy().astype(np.int64)
    nv = len(v)
    t1 = time.perf_counter()
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    adj = coo_matrix((np.ones(2 * len(a), np.int8), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(nv, nv)).tocsr()
    adj.data[:] = 1                                             # (duplicates were summed: distinct neighbours count once)
    t2 = time.perf_counter()
    p = v[f]
    e1, e2 = np.roll(p, -1, axis=1) - p, np.roll(p, -2, axis=1) - p
    cr = np.cross(e1, e2)
    s = np.linalg.norm(cr, axis=2)
    angle = np.arctan2(s, (e1 * e2).sum(2))
    unit = cr[:, 0] / np.maximum(s[:, :1], 1e-300)
    t3 = time.perf_counter()
    n = np.zeros((nv, 3))
    np.add.at(n, f.reshape(-1), (angle[:, :, None] * unit[:, None, :]).reshape(-1, 3))
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    t4 = time.perf_counter()
    deg = np.maximum(np.asarray(adj.sum(1)).reshape(-1, 1), 1)
    x = v + 0.5 * ((adj.astype(np.float64) @ v) / deg - v)
    t5 = time.perf_counter()
    return {'copy': (t1 - t0) * 1e3, 'adjacency': (t2 - t1) * 1e3, 'face_pass': (t3 - t2) * 1e3, 'normals': (t4 - t3) * 1e3,
            'smooth_step': (t5 - t4) * 1e3}, {'directed_entries': int(adj.nnz), 'checksum': float(np.abs(x).sum() + np.abs(n).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy / scipy timing')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mesh = case_mesh(dev, 1_000_000, (40.0, 40.0, 10.0), 8)
    t = MeshTopology(mesh.v, mesh.f)
    stages(t)                                                           # warm-up
    runs = [stages(t) for _ in range(args.reps)]
    g = runs[0][1]
    nv, nd = g.n_vertices, int(g.neighbours.shape[0])
    rec = {'vertices': nv, 'faces': g.n_faces, 'directed_entries': nd, 'boundary_vertices': int((g.vertex_kind == 1).sum()),
           'max_degree': int(g.vertex_degree.max()), 'state_row_bytes': 24,
           'gpu_ms': {k: float(np.median([r[0][k] for r in runs])) for k in runs[0][0]}}
    rec['step_model_bytes'] = step_bytes(nv, nd)
    rec['step_model_gb_per_s'] = rec['step_model_bytes'] / (rec['gpu_ms']['smooth_step'] * 1e-3) / 1e9
    if not args.no_host:
        rec['host_ms'], rec['host_info'] = host_path(mesh)
    print('configs2', json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump({'configs2': rec}, fh, indent=1)


if __name__ == '__main__':
    main()
