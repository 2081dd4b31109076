"""Per-stage times of the GPU mesh cross-sections (nksr_amd/mesh_slice.py, csrc/meshslice.hip).

    python -m nksr_amd.tools.prof_mesh_slice [--json OUT] [--md OUT] [--reps 20] [--no-host] [--host-max-segments 8000000]

Case: the configs[2] mesh of tools/prof_mesh_simplify (1 M-point synth_scene, detail_level 1.0, extract_dual_mesh(mise_iter=1)), ~2.3 M
triangles; 1, 10, 100 and 1000 levels along z, spread evenly inside the mesh's height range, and one oblique plane through the centre of
its box.  Stages (HIP events round the stages of ``MeshSlicer.slice``, median of --reps warm runs): heights, counts (both range
kernels' launch, the two scans and the read of N and S), points, segments, rank (the doubling rounds, the scan of the representative
flags and the read of L), polylines (the representative list, its sort by plane, the sizes, their scans, the fill) and measures (four
by-key scans and the plane tables).  The two size reads sit inside 'counts' and 'rank': the host waits there, the GPU does not idle
elsewhere.  The points kernel is timed in both shapes (one lane per edge, one lane per point), and the counts kernel alone, in windows of
BATCH launches back to back (a single launch of 20-200 us is too short a window); a whole ``slice`` is 60-odd launches, so below about
a millisecond its stages measure launches, not bytes, and the inputs of a repeated run come from the caches, not from HBM.  The byte
model of the face pass (``face_pass_bytes``): what 'counts' and 'segments' must move at least per face, per crossing face, per edge
and per segment.  'host'
is the same work in vectorised numpy on the host (np.unique edge table, np.searchsorted ranges, the same successor gather and the same
pointer doubling), with the copy to the host before it; it is skipped above --host-max-segments segments.
"""
import argparse
import json
import time

import numpy as np
import torch

from nksr_amd import mesh_slice as sl
from nksr_amd.tools.prof_mesh_simplify import case_mesh

LEVELS = (1, 10, 100, 1000)
BATCH = 20          # launches per timed window where one kernel is timed alone


def stages(s, normal, offsets):
    ev = [torch.cuda.Event(enable_timing=True)]
    ev[0].record()

    def mark(stage):
        ev.append(torch.cuda.Event(enable_timing=True))
        ev[-1].record()
    r = s.slice(normal, offsets, _mark=mark)
    torch.cuda.synchronize()
    return {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(sl.STAGES)}, r


def points_both_ways(s, r, reps):
    """Median milliseconds of nksr_slice_points with one lane per edge and with one lane per point."""
    t = s.topology
    lo_f, seg_start, lo_e, point_start = sl.plane_ranges(r.vertex_height, s.f, t.face_valid, t.edges, r.offsets)
    times = {'by_edge': [], 'by_point': []}
    for _ in range(reps + 1):                           # the two shapes alternate; a window is BATCH launches back to back
        for name, by_point in (('by_edge', 0), ('by_point', 1)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                sl.edge_points(s.x, r.vertex_height, t.edges, r.offsets, lo_e, point_start, r.n_points, by_point=by_point)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / BATCH)
    return {name: float(np.median(v[1:])) for name, v in times.items()}


def face_pass_bytes(nf, ne, crossing_faces, ns, index_bytes):
    """Bytes the byte model charges 'counts' + 'segments'.  counts, per face: three indices, three heights, the validity byte, lo (4 B)
    and the count (8 B) out; per edge: its vertex pair (8 B), two heights, lo and the count out.  segments, per face: its scanned start
    (8 B); per crossing face: three indices, three heights, three half-edge edges (12 B), lo (4 B); per segment: the offset (8 B), of its
    two edges point_start, lo and class (2 x 13 B), of its two neighbours the face (4 B), seg_start and lo (2 x 16 B), and 24 B out."""
    counts = nf * (3 * index_bytes + 24 + 1 + 12) + ne * (8 + 16 + 12)
    segments = nf * 8 + crossing_faces * (3 * index_bytes + 24 + 12 + 4) + ns * (8 + 26 + 32 + 24)
    return counts, segments


def host_path(mesh, normal, offsets):
    """The same sections on the host in vectorised numpy (milliseconds per step); the mesh of the case has no invalid face."""
    t0 = time.perf_counter()
    x, f = mesh.v.cpu().numpy().astype(np.float64), mesh.f.cpu().numpy().astype(np.int64)
    o, n = np.asarray(offsets, np.float64), np.asarray(normal, np.float64)
    t1 = time.perf_counter()
    nf = len(f)
    a, b = f, np.roll(f, -1, axis=1)
    key = ((np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1)
    uk, he_edge, count = np.unique(key, return_inverse=True, return_counts=True)
    he_edge = he_edge.reshape(-1)
    order = np.argsort(he_edge, kind='stable')
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    two = count == 2
    adj = np.full(3 * nf, -1, np.int64)
    h0, h1 = order[first[two]], order[first[two] + 1]
    adj[h0], adj[h1] = h1 // 3, h0 // 3
    interior = two.copy()
    interior[two] = (a.reshape(-1)[h0] < b.reshape(-1)[h0]) != (a.reshape(-1)[h1] < b.reshape(-1)[h1])
    t2 = time.perf_counter()
    h = x @ n
    ea, eb = uk >> 32, uk & 0xFFFFFFFF
    lo_e = np.searchsorted(o, np.minimum(h[ea], h[eb]), side='right')
    cnt_e = np.searchsorted(o, np.maximum(h[ea], h[eb]), side='right') - lo_e
    point_start = np.concatenate([[0], np.cumsum(cnt_e)])
    pe = np.repeat(np.arange(len(uk)), cnt_e)
    pj = np.arange(point_start[-1]) - point_start[pe] + lo_e[pe]
    t = (o[pj] - h[ea[pe]]) / (h[eb[pe]] - h[ea[pe]])
    pts = x[ea[pe]] + t[:, None] * (x[eb[pe]] - x[ea[pe]])
    t3 = time.perf_counter()
    hc = h[f]
    lo_f = np.searchsorted(o, hc.min(1), side='right')
    cnt_f = np.searchsorted(o, hc.max(1), side='right') - lo_f
    seg_start = np.concatenate([[0], np.cumsum(cnt_f)])
    sf = np.repeat(np.arange(nf), cnt_f)
    sj = np.arange(seg_start[-1]) - seg_start[sf] + lo_f[sf]
    up = hc[sf] >= o[sj, None]
    nxt = np.roll(up, -1, axis=1)
    kd, ku = np.argmax(up & ~nxt, axis=1), np.argmax(~up & nxt, axis=1)
    ed, eu = he_edge[3 * sf + kd], he_edge[3 * sf + ku]
    tail, head = point_start[ed] + sj - lo_e[ed], point_start[eu] + sj - lo_e[eu]
    g = adj[3 * sf + kd]
    pred = np.where(interior[ed], seg_start[g] + sj - lo_f[g], -1)
    t4 = time.perf_counter()
    ns = len(sf)
    s = np.arange(ns)
    link = pred >= 0
    px, py, pz, pw = np.where(link, pred, s), link.astype(np.int64), s.copy(), np.zeros(ns, np.int64)
    rounds = sl.chain_rank_rounds(ns) if ns else 0
    for k in range(rounds):
        act = px != s
        bz = pz[px]
        upd = act & (bz < pz)
        pw = np.where(upd, (1 << k) + pw[px], pw)
        pz = np.where(upd, bz, pz)
        py = np.where(act, py + py[px], py)
        px = np.where(act, px[px], px)
    is_open = pred[px] < 0 if ns else np.zeros(0, bool)
    rep, rank = np.where(is_open, px, pz), np.where(is_open, py, pw)
    t5 = time.perf_counter()
    reps = np.nonzero(rep == s)[0]
    reps = reps[np.argsort(sj[reps], kind='stable')]
    poly_of = np.empty(ns, np.int64)
    poly_of[reps] = np.arange(len(reps))
    sp = poly_of[rep]
    pos = np.argsort(sp * ns + rank)                    # segments in polyline order
    d = pts[head[pos]] - pts[tail[pos]]
    length = np.bincount(sp[pos], weights=np.sqrt((d * d).sum(1)), minlength=len(reps))
    t6 = time.perf_counter()
    return ({'copy': (t1 - t0) * 1e3, 'edge_table': (t2 - t1) * 1e3, 'points': (t3 - t2) * 1e3, 'segments': (t4 - t3) * 1e3, 'rank': (t5 - t4) * 1e3,
             'polylines': (t6 - t5) * 1e3, 'total': (t6 - t0) * 1e3},
            {'n_points': int(point_start[-1]), 'n_segments': int(ns), 'n_polylines': int(len(reps)), 'total_length': float(length.sum())})


def markdown(out):
    first = next(iter(out.values()))
    lines = ['# Mesh cross-sections: per-stage times', '',
             '`python -m nksr_amd.tools.prof_mesh_slice --md profiles/mesh_slice.md` on one MI355X: HIP-event medians of %d warm runs,' % first['reps'],
             'milliseconds.  The mesh is the configs[2] mesh (1 M-point `synth_scene`, `detail_level=1.0`, `extract_dual_mesh(mise_iter=1)`):',
             '%d vertices, %d triangles, %d unique edges, fp32 positions, int64 faces.  The levels are spread evenly inside the z range;' % (
                 first['vertices'], first['faces'], first['edges']),
             '"oblique" is one plane with normal (1, 2, 3) through the centre of the box.  The reads of N and S are inside `counts`, the read',
             'of L inside `rank`.  "host" is the same work in vectorised numpy on the host, the copy included.', '',
             '| run | N | S | L | rounds | ' + ' | '.join(sl.STAGES) + ' | GPU total | host total |', '|' + '---|' * (len(sl.STAGES) + 7)]
    for name, r in out.items():
        lines.append('| %s | %d | %d | %d | %d | ' % (name, r['n_points'], r['n_segments'], r['n_polylines'], r['rounds']) +
                     ' | '.join('%.3f' % r['gpu_ms'][k] for k in sl.STAGES) +
                     ' | %.3f | %s |' % (r['gpu_ms']['total'], '%.0f' % r['host_ms']['total'] if 'host_ms' in r else 'not timed'))
    lines += ['', '**Share of the ranking pass.** `rank` over the GPU total: ' +
              ', '.join('%s %.0f %%' % (name, 100 * r['gpu_ms']['rank'] / r['gpu_ms']['total']) for name, r in out.items()) + '.',
              'A round reads 16 B, gathers 16 B and writes 16 B per segment: ' +
              ', '.join('%s %d rounds x %d x 48 B = %.0f MB, %.0f GB/s over the stage' % (
                  name, r['rounds'], r['n_segments'], r['rounds'] * r['n_segments'] * 48 / 1e6, r['rounds'] * r['n_segments'] * 48 / r['gpu_ms']['rank'] / 1e6)
                  for name, r in out.items() if r['n_planes'] >= 100) + '.', '',
              '**The points kernel in its two shapes** (same outputs, bit for bit; alternating windows of %d launches):' % BATCH, '', '| run | N | one lane per edge | one lane per point |', '|---|---|---|---|']
    for name, r in out.items():
        lines.append('| %s | %d | %.3f | %.3f |' % (name, r['n_points'], r['points_ms']['by_edge'], r['points_ms']['by_point']))
    lines += ['', '`MeshSlicer` uses one lane per %s (`mesh_slice.POINTS_BY_POINT`).  On this mesh an edge crosses at most a few planes; a coarse mesh' % (
        'point' if sl.POINTS_BY_POINT else 'edge'), 'under many levels (long per-edge loops, strided stores) has not been measured.']
    lines += ['', '**Byte model of the face pass** (`counts` + `segments`).  `counts`, per face: three indices (%d B each), three heights, the validity byte,' % first['index_bytes'],
              '12 B out; per edge: 8 B, two heights, 12 B out.  `segments`, per face: 8 B of its scanned start; per crossing face: three indices,',
              'three heights, 12 B of half-edge edges, 4 B; per segment: 8 B offset, 2 x 13 B of its edges, 2 x 16 B of its neighbours and 24 B out.',
              'The counts kernel is timed alone, %d launches per window (`counts` the stage also holds two scans and a host read); the' % BATCH,
              'repeated runs find their inputs in the caches, so the rates are cache rates, not HBM rates.', '',
              '| run | crossing faces | counts bytes | counts kernel ms | GB/s | segments bytes | segments ms | GB/s |', '|---|---|---|---|---|---|---|---|']
    for name, r in out.items():
        lines.append('| %s | %d | %d | %.3f | %.0f | %d | %.3f | %.0f |' % (
            name, r['crossing_faces'], r['counts_model_bytes'], r['counts_kernel_ms'], r['counts_model_bytes'] / r['counts_kernel_ms'] / 1e6,
            r['segments_model_bytes'], r['gpu_ms']['segments'], r['segments_model_bytes'] / max(r['gpu_ms']['segments'], 1e-9) / 1e6))
    if any('host_ms' in r for r in out.values()):
        lines += ['', '| run | host copy | edge table | points | segments | rank | polylines |', '|---|---|---|---|---|---|---|']
        for name, r in out.items():
            if 'host_ms' in r:
                lines.append('| %s | ' % name + ' | '.join('%.0f' % r['host_ms'][k] for k in ('copy', 'edge_table', 'points', 'segments', 'rank', 'polylines')) + ' |')
    return '\n'.join(lines) + '\n'


def counts_kernel_ms(s, r, reps):
    t = s.topology
    nf, ne, dev = s.n_faces, t.edges.shape[0], s.device
    lo_f, lo_e = torch.empty(nf, dtype=torch.int32, device=dev), torch.empty(ne, dtype=torch.int32, device=dev)
    cnt_f, cnt_e = torch.empty(nf + 1, dtype=torch.int64, device=dev), torch.empty(ne + 1, dtype=torch.int64, device=dev)
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BATCH):
                sl.call('nksr_slice_counts', sl.ptr(r.vertex_height), s.n_vertices, sl.ptr(s.f), sl.is64(s.f), nf, sl.ptr(t.face_valid), sl.ptr(t.edges), ne,
                    sl.ptr(r.offsets), r.n_planes, sl.ptr(lo_f), sl.ptr(cnt_f), sl.ptr(lo_e), sl.ptr(cnt_e), sl.stream())
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / BATCH)
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the tables as markdown')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy timing')
    ap.add_argument('--host-max-segments', type=int, default=8_000_000)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mesh, _ = case_mesh(dev)
    s = sl.MeshSlicer(mesh.v, mesh.f)
    lo, hi = mesh.v.double().amin(0).cpu().numpy(), mesh.v.double().amax(0).cpu().numpy()
    runs = [('%d levels' % p, (0.0, 0.0, 1.0), lo[2] + (hi[2] - lo[2]) * (np.arange(p) + 0.5) / p) for p in LEVELS]
    oblique = np.array(s._unit((1.0, 2.0, 3.0)))
    runs.append(('oblique', tuple(oblique), np.array([float(oblique @ (0.5 * (lo + hi)))])))
    out = {}
    for name, normal, offsets in runs:
        stages(s, normal, offsets)                                      # warm-up
        got = [stages(s, normal, offsets) for _ in range(args.reps)]
        r = got[0][1]
        rec = {'vertices': s.n_vertices, 'faces': s.n_faces, 'edges': int(s.topology.num_edges), 'reps': args.reps, 'index_bytes': s.f.element_size(),
               'n_planes': r.n_planes, 'n_points': r.n_points, 'n_segments': r.n_segments, 'n_polylines': r.n_polylines, 'rounds': r.rounds,
               'open_polylines': int(r.plane_open.sum().item()), 'total_length': float(r.plane_length.sum().item()),
               'crossing_faces': int((r.seg_start[1:] > r.seg_start[:-1]).sum().item()),
               'gpu_ms': {k: float(np.median([g[0][k] for g in got])) for k in sl.STAGES}}
        rec['gpu_ms']['total'] = sum(rec['gpu_ms'].values())
        rec['points_ms'] = points_both_ways(s, r, args.reps)
        rec['counts_kernel_ms'] = counts_kernel_ms(s, r, args.reps)
        rec['counts_model_bytes'], rec['segments_model_bytes'] = face_pass_bytes(s.n_faces, rec['edges'], rec['crossing_faces'], r.n_segments, rec['index_bytes'])
        if not args.no_host and r.n_segments <= args.host_max_segments:
            torch.cuda.synchronize()
            rec['host_ms'], rec['host_info'] = host_path(mesh, r.normal, r.offsets.cpu().numpy())
            rec['host_agrees'] = all(rec['host_info'][k] == rec[k] for k in ('n_points', 'n_segments', 'n_polylines'))      # (its heights are numpy's)
        del r, got
        out[name] = rec
        print(name.replace(' ', '_'), json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(out))


if __name__ == '__main__':
    main()
