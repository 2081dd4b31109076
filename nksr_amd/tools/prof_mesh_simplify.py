"""Per-stage times of the GPU mesh simplification (nksr_amd/mesh_simplify.py, csrc/meshsimp.hip).

    python -m nksr_amd.tools.prof_mesh_simplify [--json OUT] [--md OUT] [--reps 5] [--no-host]

Case: the configs[2] mesh of tools/prof_mesh_topology (1 M-point synth_scene, detail_level 1.0, extract_dual_mesh(mise_iter=1)),
~2.3 M triangles, with an fp32 [V, 3] colour, at cell sizes of 2, 4 and 8 voxels.  Stages (HIP events, median of --reps warm runs; the
read-back of K is inside 'clusters'): cell keys, clusters (sort, then the run table of ops.sorted_runs), the face remap, the duplicate
pass (two sorts and the comparison), the corner incidence of the clusters (keys, sort, row starts), the placement (k_simp_place, the
hot kernel), the colour means and the final compaction.  The byte model of the placement: per corner three position rows and the 4 B
corner id, per cluster its two run starts (8 B) and 24 B out -- what the kernel must move at least; the three face indices of a corner
(24 B with int64 faces) and the vertex run of the mean come on top and are served mostly by the caches.  'host_ms' is the same work
in numpy on the host (np.floor, np.unique, np.add.at, a batched np.linalg.solve), with the copy to the host before it.
"""
import argparse
import json
import time

import numpy as np
import torch

from nksr_amd import mesh_simplify as ms
from nksr_amd.mesh_topology import compact_mesh

VOXELS = (2, 4, 8)
STAGES = ['cell_keys', 'clusters', 'face_remap', 'duplicates', 'corner_incidence', 'place', 'colour_means', 'compaction']


def stages(s, h):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
    origin, bits = s._grid(h, None)
    ev[0].record()
    keys, ids, _ = ms.cell_keys(s.x, s.vertex_ref, origin, h)
    ev[1].record()
    c = ms.clusters(keys, ids, bits)
    ev[2].record()
    m = ms.face_remap(s.f, s.n_vertices, c.cluster_of)
    ev[3].record()
    keep, dups = ms.flag_duplicates(m, c.n)
    ev[4].record()
    corners = ms.corner_incidence(m.cluster_faces, m.valid, c.n)
    ev[5].record()
    rep = ms.place(s.x, s.f, corners, c, origin, h, 1e-3, ms.SIMP_QUADRIC)
    ev[6].record()
    means = ms.cluster_means(s.colors, c)
    ev[7].record()
    v2, f2, _, _ = compact_mesh(rep, m.cluster_faces, keep, means)
    ev[8].record()
    torch.cuda.synchronize()
    out = {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(STAGES)}
    n_corners = int(corners[0][c.n].item()) & 0xFFFFFFFF
    info = {'clusters': c.n, 'corners': n_corners, 'longest_corner_row': int(((corners[0][1:].long() & 0xFFFFFFFF) - (corners[0][:-1].long() & 0xFFFFFFFF)).max()),
            'vertices_out': int(v2.shape[0]), 'faces_out': int(f2.shape[0]), 'duplicate_faces': int(dups.item())}
    return out, info


def place_bytes(n_corners, n_clusters, row_bytes):
    """Bytes the byte model charges the placement kernel."""
    return n_corners * (3 * row_bytes + 4) + n_clusters * (8 + 24)


def host_path(mesh, h):
    """The same result on the host (milliseconds per step; the mesh of the case has no invalid face)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, f = mesh.v.cpu().numpy().astype(np.float64), mesh.f.cpu().numpy().astype(np.int64)
    t1 = time.perf_counter()
    origin = x.min(0)
    idx = np.floor((x - origin) / h).astype(np.int64)
    keys, cid = np.unique((idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2], return_inverse=True)
    cid = cid.reshape(-1)
    nk = len(keys)
    t2 = time.perf_counter()
    g = cid[f]
    alive = np.nonzero((g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2]))[0]
    t = np.sort(g[alive], axis=1)
    if nk < (1 << 21):                                                  # the sorted triple fits one word
        _, first = np.unique((t[:, 0] << 42) | (t[:, 1] << 21) | t[:, 2], return_index=True)
    else:
        _, first = np.unique(t, axis=0, return_index=True)
    kept = g[alive[np.sort(first)]]
    t3 = time.perf_counter()
    centre = origin + (np.stack([keys >> 42, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF], 1) + 0.5) * h
    s = np.zeros((nk, 3))
    np.add.at(s, cid, x - centre[cid])
    mean = s / np.bincount(cid, minlength=nk)[:, None]
    p = x[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    ok = length > 0
    unit, area = n[ok] / length[ok, None], 0.5 * length[ok]
    outer = (area[:, None, None] * unit[:, :, None] * unit[:, None, :]).reshape(-1, 9)
    a_mat, b_vec = np.zeros((nk, 9)), np.zeros((nk, 3))
    for k in range(3):
        c = g[ok, k]
        d = -(unit * (p[ok, 0] - centre[c])).sum(1)
        np.add.at(a_mat, c, outer)
        np.add.at(b_vec, c, (area * d)[:, None] * unit)
    t4 = time.perf_counter()
    a_mat = a_mat.reshape(nk, 3, 3)
    tau = np.trace(a_mat, axis1=1, axis2=2)
    flat = ~(tau > 0)
    m = a_mat + (1e-3 * tau)[:, None, None] * np.eye(3) + flat[:, None, None] * np.eye(3)
    sol = np.linalg.solve(m, (-b_vec + (1e-3 * tau)[:, None] * mean)[:, :, None])[:, :, 0]
    rep = centre + np.clip(np.where(flat[:, None], mean, sol), -0.5 * h, 0.5 * h)
    t5 = time.perf_counter()
    return {'copy': (t1 - t0) * 1e3, 'clusters': (t2 - t1) * 1e3, 'faces': (t3 - t2) * 1e3, 'quadrics': (t4 - t3) * 1e3, 'solve': (t5 - t4) * 1e3,
            'total': (t5 - t0) * 1e3}, {'clusters': nk, 'faces_out': len(kept), 'checksum': float(np.abs(rep).sum())}


def case_mesh(dev):
    """(mesh, voxel size in the cloud's units) of the configs[2] case."""
    import nksr_amd
    from nksr_amd import utils
    xyz, nrm = utils.synth_scene(1_000_000, seed=0, extent=(40.0, 40.0, 10.0), n_objects=8)
    rec = nksr_amd.Reconstructor(dev)
    fld = rec.reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), detail_level=1.0)
    return fld.extract_dual_mesh(mise_iter=1), rec.hparams.voxel_size / fld.scale


def markdown(out):
    first = next(iter(out.values()))
    lines = ['# Mesh simplification: per-stage times', '',
             '`python -m nksr_amd.tools.prof_mesh_simplify --md profiles/mesh_simplify.md` on one MI355X: HIP-event medians of %d warm runs,' % first['reps'],
             'milliseconds.  The mesh is the configs[2] mesh (1 M-point `synth_scene`, `detail_level=1.0`, `extract_dual_mesh(mise_iter=1)`):',
             '%d vertices, %d triangles, fp32 positions, int64 faces, an fp32 [V, 3] colour; voxel %.6g.  "host" is the numpy restatement of' % (
                 first['vertices'], first['faces'], first['voxel']),
             'the same work on the host.', '']
    lines += ['| cell | K | faces out | longest corner row | ' + ' | '.join(STAGES) + ' | GPU total | host total |', '|' + '---|' * (len(STAGES) + 6)]
    for name, r in out.items():
        lines.append('| %s | %d | %d | %d | ' % (name, r['clusters'], r['faces_out'], r['longest_corner_row']) +
                     ' | '.join('%.3f' % r['gpu_ms'][k] for k in STAGES) +
                     ' | %.3f | %s |' % (r['gpu_ms']['total'], '%.0f' % r['host_ms']['total'] if 'host_ms' in r else 'not timed'))
    lines += ['', '**Byte model of `k_simp_place`.** Per corner three position rows (%d B each) and the 4 B corner id, per cluster two run starts (8 B)' % first['row_bytes'],
              'and 24 B out.', '', '| cell | corners | model bytes | place ms | modelled GB/s |', '|---|---|---|---|---|']
    for name, r in out.items():
        lines.append('| %s | %d | %d | %.3f | %.0f |' % (name, r['corners'], r['place_model_bytes'], r['gpu_ms']['place'], r['place_model_gb_per_s']))
    if 'host_ms' in first:
        lines += ['', '| cell | host copy | clusters | faces | quadrics | solve |', '|---|---|---|---|---|---|']
        for name, r in out.items():
            lines.append('| %s | ' % name + ' | '.join('%.0f' % r['host_ms'][k] for k in ('copy', 'clusters', 'faces', 'quadrics', 'solve')) + ' |')
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the tables as markdown')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy timing')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mesh, voxel = case_mesh(dev)
    colour = torch.rand((mesh.v.shape[0], 3), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(0))
    s = ms.MeshSimplifier(mesh.v, mesh.f, colour)
    out = {}
    for k in VOXELS:
        h = k * voxel
        stages(s, h)                                                    # warm-up
        runs = [stages(s, h) for _ in range(args.reps)]
        rec = {'vertices': s.n_vertices, 'faces': s.n_faces, 'voxel': voxel, 'cell_size': h, 'reps': args.reps, 'row_bytes': 3 * s.x.element_size(),
               **runs[0][1], 'gpu_ms': {n: float(np.median([r[0][n] for r in runs])) for n in STAGES}}
        rec['gpu_ms']['total'] = sum(rec['gpu_ms'].values())
        rec['place_model_bytes'] = place_bytes(rec['corners'], rec['clusters'], rec['row_bytes'])
        rec['place_model_gb_per_s'] = rec['place_model_bytes'] / (rec['gpu_ms']['place'] * 1e-3) / 1e9
        if not args.no_host:
            rec['host_ms'], host_info = host_path(mesh, h)
            assert host_info['clusters'] == rec['clusters'] and host_info['faces_out'] == rec['faces_out'], (host_info, rec)
            rec['host_checksum'] = host_info['checksum']
        out['%d voxels' % k] = rec
        print('%d_voxels' % k, json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(out))


if __name__ == '__main__':
    main()
