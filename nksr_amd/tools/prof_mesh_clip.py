"""Per-stage times of the GPU mesh clipper (nksr_amd/mesh_clip.py, csrc/meshclip.hip).

    python -m nksr_amd.tools.prof_mesh_clip [--json OUT] [--md OUT] [--reps 20] [--tiles 16]

Case: the configs[2] mesh of tools/prof_mesh_simplify (1 M-point synth_scene, detail_level 1.0, extract_dual_mesh(mise_iter=1)), ~2.3 M
triangles, with its vertex positions as a three-channel attribute; 1, 10, 100 and 1000 planes along z, spread evenly inside the mesh's
height range, and a tile set of --tiles x --tiles tiles over its x-y box.  Stages (HIP events round the stages of ``MeshClipper.split``,
median of --reps warm runs): heights, counts (the range kernel, three scans and the read of N, F2 and the piece count), points, faces
(nksr_clip_faces), attr (nksr_clip_attr and the concatenation) and group (``SplitMesh.parts()``: the corner keys, two sorts, the run
table and its read, the face gather), timed after the split.  The yardsticks: ``MeshSlicer.slice`` on the same mesh and planes (the
parent's cost of the shared stages heights, counts and points, plus its segments and polylines), and the byte model of the face kernel
(``face_kernel_bytes``) against the time of that kernel alone, in both shapes, in alternating windows of BATCH launches back to back.
A repeated run finds its inputs in the caches, so the rates are cache rates where the arrays fit, not HBM rates.  The host has no
vectorised restatement of the face pass (tests/mesh_clip_ref.py is plain loops); it is not timed.
"""
import argparse
import json

import numpy as np
import torch

from nksr_amd import mesh_clip as cl
from nksr_amd import mesh_slice as sl
from nksr_amd.tools.prof_mesh_simplify import case_mesh

PLANES = (1, 10, 100, 1000)
BATCH = 20          # launches per timed window where one kernel is timed alone


def stages(c, normal, offsets):
    ev = [torch.cuda.Event(enable_timing=True)]
    ev[0].record()

    def mark(stage=None):
        ev.append(torch.cuda.Event(enable_timing=True))
        ev[-1].record()
    r = c.split(normal, offsets, _mark=mark)
    r.parts()
    mark()
    torch.cuda.synchronize()
    return {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(cl.STAGES)}, r


def faces_both_ways(c, r, reps):
    """Median milliseconds of nksr_clip_faces with one lane per face and with one lane per (face, piece)."""
    s, t = c.slicer, c.topology
    _, seg_start, _, point_start = sl.plane_ranges(r.vertex_height, s.f, t.face_valid, t.edges, r.offsets)
    face_start, piece_start = cl.face_starts(t.face_valid, seg_start)
    n_pieces = int(piece_start[-1].item())
    times = {'by_face': [], 'by_piece': []}
    for _ in range(reps + 1):
        for name, by_piece in (('by_face', 0), ('by_piece', 1)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                cl.clip_faces(r.vertex_height, s.f, t.face_valid, s.halfedge_edge, point_start, r.n_points, r.offsets, face_start, piece_start, n_pieces,
                              r.n_faces, by_piece=by_piece)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / BATCH)
    return {name: float(np.median(v[1:])) for name, v in times.items()}, n_pieces


def face_kernel_bytes(nf, n_out, index_bytes):
    """Bytes the byte model charges nksr_clip_faces (one lane per face).  Per face: the validity byte, three indices, three heights (24 B,
    gathered), three half-edge edges (12 B), their three point_start entries (24 B, gathered) and face_start (8 B); per output triangle:
    12 B of indices, 4 B of source and 4 B of part.  The offsets are read once per workgroup into LDS (or searched in place above 2048
    planes) and are not charged."""
    return nf * (1 + 3 * index_bytes + 24 + 12 + 24 + 8) + n_out * 20


def slice_ms(s, normal, offsets, reps):
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.slice(normal, offsets)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times[1:]))


def tiles_ms(c, size, origin, reps):
    times, t = [], None
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t = c.tiles(size, origin)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times[1:])), t


def markdown(out, tiles):
    first = next(iter(out.values()))
    shape = 'one lane per (face, piece)' if cl.FACES_BY_PIECE else 'one lane per face'
    lines = ['# Mesh clipping: per-stage times', '',
             '`python -m nksr_amd.tools.prof_mesh_clip --md profiles/mesh_clip.md` on one MI355X: HIP-event medians of %d warm runs,' % first['reps'],
             'milliseconds.  The mesh is the configs[2] mesh (1 M-point `synth_scene`, `detail_level=1.0`, `extract_dual_mesh(mise_iter=1)`):',
             '%d vertices, %d triangles, %d unique edges, fp32 positions, int64 faces, three fp32 attribute channels.  The planes are' % (
                 first['vertices'], first['faces'], first['edges']),
             'spread evenly inside the z range.  The read of N, F2 and the piece count is inside `counts`; `group` is `SplitMesh.parts()`.',
             '`slice` is `MeshSlicer.slice` on the same mesh and planes: the parent\'s cost of heights, counts and points plus its own',
             'segments and polylines.  The host has no vectorised restatement of the face pass and is not timed.', '',
             '| run | N | F2 | ' + ' | '.join(cl.STAGES) + ' | split total | with group | slice |', '|' + '---|' * (len(cl.STAGES) + 6)]
    for name, r in out.items():
        g = r['gpu_ms']
        lines.append('| %s | %d | %d | ' % (name, r['n_points'], r['n_faces']) + ' | '.join('%.3f' % g[k] for k in cl.STAGES) +
                     ' | %.3f | %.3f | %.3f |' % (g['total'] - g['group'], g['total'], r['slice_ms']))
    lines += ['', '**The face kernel in its two shapes** (same outputs, bit for bit; alternating windows of %d launches) and its byte model:' % BATCH,
              'per face the validity byte, three indices (%d B each), three heights, 12 B of half-edge edges, 24 B of point starts and 8 B of' % first['index_bytes'],
              'its scanned start; per output triangle 20 B.  The repeated runs find their inputs in the caches where they fit.', '',
              '| run | pieces | model bytes | one lane per face ms | GB/s | one lane per piece ms | GB/s |', '|---|---|---|---|---|---|---|']
    for name, r in out.items():
        f = r['faces_ms']
        lines.append('| %s | %d | %d | %.3f | %.0f | %.3f | %.0f |' % (name, r['n_pieces'], r['model_bytes'], f['by_face'], r['model_bytes'] / f['by_face'] / 1e6,
                                                                      f['by_piece'], r['model_bytes'] / f['by_piece'] / 1e6))
    lines += ['', '`MeshClipper` uses %s (`mesh_clip.FACES_BY_PIECE`).  Compiled for gfx950 the kernel with one lane per face uses 36 VGPRs, the one' % shape,
              'with one lane per piece 30, no scratch and no spills (`-Rpass-analysis=kernel-resource-usage`); both stage the offsets in 16 KiB of LDS',
              'up to 2048 planes.']
    if tiles:
        lines += ['', '**Tile set.** `tiles` with %d x %d tiles (%d non-empty, %d faces out of %d): %.3f ms for both splits, the second' % (
            tiles['shape'][0], tiles['shape'][1], tiles['nonempty'], tiles['faces_out'], first['faces'], tiles['ms']),
                  "mesh's edge table and the grouping (median of %d warm runs)." % tiles['reps']]
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the tables as markdown')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--tiles', type=int, default=16, help='tiles per axis of the tile set (0: skip)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mesh, _ = case_mesh(dev)
    c = cl.MeshClipper(mesh.v, mesh.f, mesh.v.to(torch.float32))
    s = c.slicer
    lo, hi = mesh.v.double().amin(0).cpu().numpy(), mesh.v.double().amax(0).cpu().numpy()
    out = {}
    for p in PLANES:
        name, normal = '%d plane%s' % (p, 's' if p > 1 else ''), (0.0, 0.0, 1.0)
        offsets = lo[2] + (hi[2] - lo[2]) * (np.arange(p) + 0.5) / p
        stages(c, normal, offsets)                                      # warm-up
        got = [stages(c, normal, offsets) for _ in range(args.reps)]
        r = got[0][1]
        rec = {'vertices': c.n_vertices, 'faces': c.n_faces, 'edges': int(c.topology.num_edges), 'reps': args.reps, 'index_bytes': s.f.element_size(),
               'n_planes': p, 'n_points': r.n_points, 'n_faces': r.n_faces, 'n_dropped': r.n_dropped,
               'gpu_ms': {k: float(np.median([g[0][k] for g in got])) for k in cl.STAGES}}
        rec['gpu_ms']['total'] = sum(rec['gpu_ms'].values())
        rec['faces_ms'], rec['n_pieces'] = faces_both_ways(c, r, args.reps)
        rec['model_bytes'] = face_kernel_bytes(c.n_faces, r.n_faces, rec['index_bytes'])
        del got
        rec['slice_ms'] = slice_ms(s, normal, offsets, args.reps)
        del r
        out[name] = rec
        print(name.replace(' ', '_'), json.dumps(rec), flush=True)
    tiles = None
    if args.tiles > 0:
        size = float(max(hi[0] - lo[0], hi[1] - lo[1])) / args.tiles * (1.0 + 1e-9)
        tile_reps = max(args.reps // 4, 3)
        ms, t = tiles_ms(c, size, (float(lo[0]), float(lo[1])), tile_reps)
        tiles = {'ms': ms, 'reps': tile_reps, 'shape': list(t.shape), 'nonempty': len(t.nonempty), 'faces_out': int(t.f.shape[0]), 'tile_size': size}
        print('tiles', json.dumps(tiles), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump({'runs': out, 'tiles': tiles}, fh, indent=1)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(out, tiles))


if __name__ == '__main__':
    main()
