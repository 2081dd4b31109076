"""Per-stage times of the GPU mesh rasteriser (nksr_amd/mesh_raster.py, csrc/meshraster.hip).

    python -m nksr_amd.tools.prof_mesh_raster [--json OUT] [--md OUT] [--reps 20]

Case: the configs[2] mesh of tools/prof_mesh_simplify (1 M-point synth_scene, detail_level 1.0, extract_dual_mesh(mise_iter=1)), ~2.3 M
triangles, seen along z at pixel sizes of 2, 1 and 0.5 voxels, with its vertex positions as a three-channel attribute.  Stages (HIP
events round the stages of ``MeshRasterizer.height_map``, median of --reps warm runs): boxes (the box kernel, the scan and the read of
the candidate count), test (nksr_raster_test), compact (flag counts, scan, the read of the hit count, nksr_raster_compact), sort (the
stable pair sort, the run table with its read, pixel_start), reduce (the fills and nksr_raster_reduce); then sample, gradient and
hillshade on the result.  The yardsticks: ``MeshSlicer.slice`` at 100 levels on the same mesh, the numpy restatement
(tests/mesh_raster_ref.py, where the checkout has it) on a subsample, as time per (face, pixel) test, and the byte model of the test
kernel (``cover_kernel_bytes``) against the time of that kernel alone in windows of BATCH launches back to back.  A repeated run finds
its inputs in the caches where they fit, so the rates are cache rates there, not HBM rates.  The register counts come from the
compiler's own resource report of csrc/meshraster.hip.
"""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import tempfile
import time

import numpy as np
import torch

from nksr_amd import build
from nksr_amd import mesh_raster as mr
from nksr_amd.mesh_slice import MeshSlicer
from nksr_amd.tools.prof_mesh_simplify import case_mesh

PIXELS = (2.0, 1.0, 0.5)        # in voxels
BATCH = 20                      # launches per timed window where one kernel is timed alone
DERIVED = ('sample', 'gradient', 'hillshade')
HOST_FACES, HOST_GRID = 2000, 64


def stages(r, pixel):
    ev = [torch.cuda.Event(enable_timing=True)]
    ev[0].record()

    def mark(stage=None):
        ev.append(torch.cuda.Event(enable_timing=True))
        ev[-1].record()
    hm = r.height_map(pixel, _mark=mark)
    hm.sample()
    mark()
    hm._horn((0.0, 0.0, 1.0))
    mark()
    hm.hillshade()
    mark()
    torch.cuda.synchronize()
    return {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(mr.STAGES + DERIVED)}, hm


def cover_kernel_ms(r, hm, reps):
    """Median milliseconds of nksr_raster_test alone."""
    _, box, cand_start = mr.face_boxes(r.x, r.f, hm._g)
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BATCH):
            mr.cover_candidates(r.x, r.f, hm._g, box, cand_start, hm.n_candidates)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / BATCH)
    return float(np.median(times[1:]))


def cover_kernel_bytes(n_cand, index_bytes, coord_bytes):
    """Bytes the byte model charges nksr_raster_test per candidate: 8 B of scanned start (what the block stages, amortised over its
    lanes, plus the lane's own read of its face's start), three indices, nine coordinates, and 9 B out (the flag and the height).  The
    16 B of the face's box are not charged: the lanes of a box share them."""
    return n_cand * (8 + 3 * index_bytes + 9 * coord_bytes + 9)


def slice_ms(mesh, reps):
    s = MeshSlicer(mesh.v, mesh.f)
    z = mesh.v[:, 2].double()
    lo, hi = float(z.min()), float(z.max())
    offsets = lo + (hi - lo) * (np.arange(100) + 0.5) / 100
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.slice((0.0, 0.0, 1.0), offsets)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times[1:]))


def host_pair_ns(mesh, pixel):
    """Nanoseconds per (face, pixel) test of the numpy restatement: HOST_FACES faces from the middle of the mesh on a HOST_GRID^2 window
    round the first of them.  None where tests/mesh_raster_ref.py is not in the checkout."""
    path = os.path.join(os.path.dirname(build.HERE), 'tests', 'mesh_raster_ref.py')
    if not os.path.exists(path):
        return None
    spec = importlib.util.spec_from_file_location('mesh_raster_ref', path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    v = mesh.v.cpu().numpy()
    f = mesh.f[mesh.f.shape[0] // 2:][:HOST_FACES].cpu().numpy()
    centre = v[f[0, 0], :2].astype(np.float64)
    origin = tuple(np.floor(centre / pixel) * pixel - HOST_GRID // 2 * pixel)
    t0 = time.perf_counter()
    ref.height_map(v, f, pixel, origin, (HOST_GRID, HOST_GRID))
    return (time.perf_counter() - t0) * 1e9 / (len(f) * HOST_GRID * HOST_GRID)


def kernel_resources():
    """{kernel: {'vgprs', 'spills', 'scratch', 'lds'}} from hipcc's resource report of csrc/meshraster.hip, or {} without a compiler."""
    if not os.path.exists(build.HIPCC):
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(build.CSRC, 'meshraster.hip'), '-o',
                                             os.path.join(tmp, 'meshraster.o')]
        text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.split('\n'):
        m = re.search(r'Function Name: _Z\d+(k_rs_[a-z_]+?)P', line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (('vgprs', r' VGPRs: (\d+)'), ('spills', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def markdown(out, extra):
    first = next(iter(out.values()))
    cols = mr.STAGES + DERIVED
    lines = ['# Mesh rasterisation: per-stage times', '',
             '`python -m nksr_amd.tools.prof_mesh_raster --md profiles/mesh_raster.md` on one MI355X: HIP-event medians of %d warm runs,' % first['reps'],
             'milliseconds.  The mesh is the configs[2] mesh (1 M-point `synth_scene`, `detail_level=1.0`, `extract_dual_mesh(mise_iter=1)`):',
             '%d vertices, %d triangles, fp32 positions, int64 faces, three fp32 attribute channels; voxel %.6g.  It is seen along z, the top' % (
                 first['vertices'], first['faces'], first['voxel']),
             'surface, on the default grid.  The size reads are inside `boxes`, `compact` and `sort`; `total` is the height map alone, without the',
             'host read of the mesh extent (once per rasteriser).  `sample` interpolates the three channels, `gradient` and `hillshade` are one',
             'launch of the Horn kernel each.', '',
             '| pixel | grid | candidates | hits | covered | max count | ' + ' | '.join(cols) + ' | total |', '|' + '---|' * (len(cols) + 7)]
    for name, r in out.items():
        g = r['gpu_ms']
        lines.append('| %s | %d x %d | %d | %d | %.1f%% | %d | ' % (name, r['shape'][0], r['shape'][1], r['n_candidates'], r['n_hits'], 100 * r['covered'],
                                                                  r['max_count']) + ' | '.join('%.3f' % g[k] for k in cols) + ' | %.3f |' % g['total'])
    lines += ['', '**The test kernel alone** (windows of %d launches) against its byte model: per candidate 8 B of scanned start, three indices' % BATCH,
              '(%d B each), nine coordinates (%d B each) and 9 B out.  The lanes of a box share one face, so most of the modelled reads are' % (
                  first['index_bytes'], first['coord_bytes']),
              'served by the caches: the rate is a cache rate, not an HBM rate.  Candidates per face: %s -- a face smaller than a pixel still' % (
                  ' / '.join('%.1f' % (r['n_candidates'] / max(r['faces'], 1)) for r in out.values())),
              'pays the nine pixels of a 3 x 3 box.', '',
              '| pixel | candidates | candidates per hit | model bytes | test kernel ms | model GB/s | ns per candidate |', '|---|---|---|---|---|---|---|']
    for name, r in out.items():
        lines.append('| %s | %d | %.1f | %d | %.3f | %.0f | %.4f |' % (name, r['n_candidates'], r['n_candidates'] / max(r['n_hits'], 1), r['model_bytes'],
                                                                      r['test_ms'], r['model_bytes'] / r['test_ms'] / 1e6,
                                                                      r['test_ms'] * 1e6 / max(r['n_candidates'], 1)))
    lines += ['', '**For scale.** `MeshSlicer.slice` at 100 levels along z on the same mesh (its edge table exists already): %.3f ms.' % extra['slice_ms']]
    if extra.get('host_pair_ns') is not None:
        lines += ['The numpy restatement (tests/mesh_raster_ref.py) on %d faces of this mesh over a %d x %d window at a pixel of one voxel:' % (
            HOST_FACES, HOST_GRID, HOST_GRID), '%.2f ns per (face, pixel) test on the host.  It tests every pair; the GPU tests the candidates of the boxes only.' %
            extra['host_pair_ns']]
    else:
        lines += ['The numpy restatement was not in the checkout and is not timed.']
    res = extra.get('resources') or {}
    if res:
        lines += ['', '**Registers** (`-Rpass-analysis=kernel-resource-usage`, gfx950):', '', '| kernel | VGPRs | VGPR spills | scratch B/lane | LDS B/block |',
                  '|---|---|---|---|---|']
        lines += ['| %s | %d | %d | %d | %d |' % (k, r.get('vgprs', -1), r.get('spills', -1), r.get('scratch', -1), r.get('lds', -1)) for k, r in res.items()]
        t = res.get('k_rs_test', {})
        if t and (t.get('vgprs', 0) > 128 or t.get('spills', 0) or t.get('scratch', 0)):
            lines += ['', 'The test kernel holds more than 128 VGPRs or spills.']
        elif t:
            lines += ['', 'The test kernel stays under 128 VGPRs and does not spill; its LDS is the staged range of scanned starts (512 entries).']
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the tables as markdown')
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mesh, voxel = case_mesh(dev)
    r = mr.MeshRasterizer(mesh.v, mesh.f, mesh.v.to(torch.float32))
    out = {}
    for k in PIXELS:
        name, pixel = '%g voxel%s' % (k, 's' if k != 1 else ''), float(k * voxel)
        stages(r, pixel)                                                # warm-up
        got = [stages(r, pixel) for _ in range(args.reps)]
        hm = got[0][1]
        rec = {'vertices': r.n_vertices, 'faces': r.n_faces, 'voxel': float(voxel), 'reps': args.reps, 'index_bytes': r.f.element_size(),
               'coord_bytes': r.x.element_size(), 'pixel': pixel, 'shape': list(hm.shape), 'n_candidates': hm.n_candidates, 'n_hits': hm.n_hits,
               'n_dropped': hm.n_dropped, 'covered': float(hm.valid.double().mean()), 'max_count': int(hm.count.max()),
               'gpu_ms': {s: float(np.median([g[0][s] for g in got])) for s in mr.STAGES + DERIVED}}
        rec['gpu_ms']['total'] = sum(rec['gpu_ms'][s] for s in mr.STAGES)
        del got
        rec['test_ms'] = cover_kernel_ms(r, hm, args.reps)
        rec['model_bytes'] = cover_kernel_bytes(hm.n_candidates, rec['index_bytes'], rec['coord_bytes'])
        del hm
        out[name] = rec
        print(name.replace(' ', '_'), json.dumps(rec), flush=True)
    extra = {'slice_ms': slice_ms(mesh, max(args.reps // 2, 3)), 'host_pair_ns': host_pair_ns(mesh, float(voxel)), 'resources': kernel_resources()}
    print('extra', json.dumps(extra), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump({'runs': out, 'extra': extra}, fh, indent=1)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(out, extra))


if __name__ == '__main__':
    main()
