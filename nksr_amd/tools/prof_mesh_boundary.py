"""Per-stage times of the GPU mesh boundary loops and hole filling (nksr_amd/mesh_boundary.py, csrc/meshbound.hip).

    python -m nksr_amd.tools.prof_mesh_boundary [--json OUT] [--md OUT] [--reps 20] [--no-host]

Cases: the configs[2] mesh of tools/prof_mesh_simplify (1 M-point synth_scene, detail_level 1.0, extract_dual_mesh(mise_iter=1)), ~2.3 M
triangles, as it is (its borders are where the mask field trimmed it), and the same mesh less the star of every 50th vertex (many small
holes).  Stages (HIP events round the stages of ``MeshBoundary.loops`` and ``MeshBoundary.fill``, median of --reps warm runs): boundary
(flags, their scan, the list), successor (the umbrella walk both ways), rank (the doubling rounds, the scan of the representative
flags, the sort of the (loop, tail) keys with its run counts, and the read of L), loops (sizes, their scans, the ordered lists and the
terms), simple (the run table and the comparison), measures (seven by-key scans, the centroid and the boxes); then the fill of
``select(max_edges=..., simple_only=False)`` by 'centroid': sizes (two scans and the size read), faces, vertices.  The edge table and the half-edge ->
edge map are the topology's and are timed apart ('topology').  The size reads sit inside 'rank' and 'sizes'.  A whole pass is some
sixty launches, so below about a millisecond its stages measure launches, not bytes, and the inputs of a repeated run come from the
caches, not from HBM.  The byte model of the successor kernel: per boundary half-edge 4 B of its id, 8 B out, and per step of either
walk a half-edge's edge (4 B), its class (1 B), the face across (4 B) and that face's three indices; of the fill kernel: per boundary
half-edge its loop, rank, tail and head (16 B), per kept one its loop's flag, size, rank and offset (13 B) and one face and its loop
out.  'host' is the same work in vectorised numpy on the host (np.unique edge table, the same walk advanced for all half-edges at once,
the same pointer doubling, np.bincount for the sums), with the copy to the host before it.
"""
import argparse
import json
import time

import numpy as np
import torch

from nksr_amd import mesh_boundary as mb
from nksr_amd._lib import TOPO_INTERIOR
from nksr_amd.mesh_topology import MeshTopology
from nksr_amd.tools.prof_mesh_simplify import case_mesh

MAX_EDGES = 16          # the holes the fill closes: a vertex star of the case mesh has at most this many edges


def _events(run, names):
    ev = [torch.cuda.Event(enable_timing=True)]
    ev[0].record()

    def mark(stage):
        ev.append(torch.cuda.Event(enable_timing=True))
        ev[-1].record()
    r = run(mark)
    torch.cuda.synchronize()
    return {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(names)}, r


def stages(b, keep=None):
    """({stage: ms} of loops() and, with ``keep``, of fill(), the BoundaryLoops)."""
    ms, r = _events(lambda mark: b.loops(_mark=mark), mb.STAGES)
    if keep is not None:
        b._loops = r
        fill_ms, _ = _events(lambda mark: b.fill(keep, 'centroid', _mark=mark), mb.FILL_STAGES)
        ms.update(('fill ' + k, x) for k, x in fill_ms.items())
    return ms, r


def topology_ms(v, f, reps):
    times = []
    for _ in range(reps + 1):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        MeshTopology(v, f).halfedge_edge
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e))
    return float(np.median(times[1:]))


def host_path(v, f):
    """The same loops on the host in vectorised numpy (milliseconds per step); the mesh of the case has no invalid face."""
    t0 = time.perf_counter()
    x, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)
    t1 = time.perf_counter()
    nf = len(f)
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    uk, he_edge, count = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_inverse=True, return_counts=True)
    he_edge = he_edge.reshape(-1)
    order = np.argsort(he_edge, kind='stable')
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    two = count == 2
    twin = np.full(3 * nf, -1, np.int64)
    h0, h1 = order[first[two]], order[first[two] + 1]
    interior = (a[h0] < b[h0]) != (a[h1] < b[h1])
    twin[h0[interior]], twin[h1[interior]] = h1[interior], h0[interior]
    t2 = time.perf_counter()
    is_b = count[he_edge] == 1
    he = np.nonzero(is_b)[0]
    nb = len(he)
    bid = np.cumsum(is_b) - 1
    nxt = lambda h: h - h % 3 + (h % 3 + 1) % 3         # noqa: E731
    cur, succ, live = nxt(he), np.full(nb, -1, np.int64), np.arange(nb)
    steps = 0
    while len(live):                                    # all walks advance together; a walk leaves when it ends
        h = cur[live]
        done = is_b[h]
        succ[live[done]] = bid[h[done]]
        go = ~done & (twin[h] >= 0)
        cur[live[go]] = nxt(twin[h[go]])
        live = live[go]
        steps += 1
    pred = np.full(nb, -1, np.int64)
    pred[succ[succ >= 0]] = np.nonzero(succ >= 0)[0]
    t3 = time.perf_counter()
    s = np.arange(nb)
    link = pred >= 0
    px, py, pz, pw = np.where(link, pred, s), link.astype(np.int64), s.copy(), np.zeros(nb, np.int64)
    rounds = int(mb.lib.nksr_chain_rank_rounds(nb)) if nb else 0
    for k in range(rounds):
        act = px != s
        bz = pz[px]
        upd = act & (bz < pz)
        pw = np.where(upd, (1 << k) + pw[px], pw)
        pz = np.where(upd, bz, pz)
        py = np.where(act, py + py[px], py)
        px = np.where(act, px[px], px)
    is_open = pred[px] < 0 if nb else np.zeros(0, bool)
    rep, rank = np.where(is_open, px, pz), np.where(is_open, py, pw)
    t4 = time.perf_counter()
    reps = np.nonzero(rep == s)[0]
    loop_of = np.searchsorted(reps, rep)
    pos = np.argsort(loop_of * max(nb, 1) + rank)       # half-edges in loop order
    p, q, p0 = x[a[he]], x[b[he]], x[a[he[rep]]]
    w = np.sqrt(((q - p) ** 2).sum(1))
    nl = len(reps)
    length = np.bincount(loop_of[pos], weights=w[pos], minlength=nl)
    area = np.stack([np.bincount(loop_of[pos], weights=(0.5 * np.cross(p - p0, q - p0))[pos, k], minlength=nl) for k in range(3)], 1)
    moment = np.stack([np.bincount(loop_of[pos], weights=(w[:, None] * 0.5 * ((p - p0) + (q - p0)))[pos, k], minlength=nl) for k in range(3)], 1)
    edges = np.bincount(loop_of, minlength=nl)
    closed = ~is_open[reps] if nb else np.zeros(0, bool)
    t5 = time.perf_counter()
    keep = closed & (edges <= MAX_EDGES)
    centroid = x[a[he[reps]]] + moment / np.maximum(length, 1e-300)[:, None]
    kept_rank = np.cumsum(keep) - 1
    sel = np.nonzero(keep[loop_of])[0]
    sel = sel[np.lexsort((rank[sel], loop_of[sel]))]            # loop by loop, in rank order
    new_f = np.stack([b[he[sel]], a[he[sel]], len(x) + kept_rank[loop_of[sel]]], 1)
    f2, v2 = np.concatenate([f, new_f]), np.concatenate([x, centroid[keep]])
    t6 = time.perf_counter()
    return ({'copy': (t1 - t0) * 1e3, 'edge_table': (t2 - t1) * 1e3, 'successor': (t3 - t2) * 1e3, 'rank': (t4 - t3) * 1e3, 'measures': (t5 - t4) * 1e3,
             'fill': (t6 - t5) * 1e3, 'total': (t6 - t0) * 1e3},
            {'n_boundary': int(nb), 'n_loops': int(nl), 'closed_loops': int(closed.sum()), 'kept_loops': int(keep.sum()), 'new_faces': int(len(new_f)),
             'walk_rounds': steps, 'total_length': float(length.sum()), 'area_norm_sum': float(np.sqrt((area ** 2).sum(1)).sum()), 'v2': int(len(v2)),
             'f2': int(len(f2))})


def less_every_nth_star(mesh, n):
    """(v, f) of ``mesh`` without the faces at the vertices 0, n, 2 n, ..."""
    gone = torch.zeros(mesh.v.shape[0], dtype=torch.bool, device=mesh.v.device)
    gone[::n] = True
    return mesh.v, mesh.f[~gone[mesh.f].any(1)].contiguous()


def markdown(out):
    names = list(mb.STAGES) + ['fill ' + k for k in mb.FILL_STAGES]
    lines = ['# Mesh boundary loops and hole filling: per-stage times', '',
             '`python -m nksr_amd.tools.prof_mesh_boundary --md profiles/mesh_boundary.md` on one MI355X: HIP-event medians of %d warm runs,' % next(iter(out.values()))['reps'],
             'milliseconds.  The mesh is the configs[2] mesh (1 M-point `synth_scene`, `detail_level=1.0`, `extract_dual_mesh(mise_iter=1)`), fp32',
             'positions, int64 faces, as it is and less the star of every 50th vertex.  `topology` is the edge table and the half-edge -> edge map',
             '(`MeshTopology`, shared with the other mesh tools); the read of L is inside `rank`, the read of the fill sizes inside `fill sizes`.',
             'The fill closes `select(max_edges=%d, simple_only=False)` by `centroid`.  "host" is the same work in vectorised numpy on the host, the copy included.' % MAX_EDGES, '',
             '| mesh | V | F | B | L | closed | kept | new faces | rounds | topology | ' + ' | '.join(names) + ' | GPU total | host total |',
             '|' + '---|' * (len(names) + 12)]
    for name, r in out.items():
        lines.append('| %s | %d | %d | %d | %d | %d | %d | %d | %d | %.3f | ' % (name, r['vertices'], r['faces'], r['n_boundary'], r['n_loops'], r['closed_loops'],
                                                                              r['kept_loops'], r['new_faces'], r['rounds'], r['topology_ms']) +
                     ' | '.join('%.3f' % r['gpu_ms'][k] for k in names) +
                     ' | %.3f | %s |' % (r['gpu_ms']['total'], '%.0f' % r['host_ms']['total'] if 'host_ms' in r else 'not timed'))
    lines += ['', '(GPU total: the stages without `topology`.)', '',
              '**Share of the ranking pass.** `rank` over the GPU total: ' +
              ', '.join('%s %.0f %%' % (name, 100 * r['gpu_ms']['rank'] / r['gpu_ms']['total']) for name, r in out.items()) + '.',
              'A round reads 16 B, gathers 16 B and writes 16 B per boundary half-edge: ' +
              ', '.join('%s %d rounds x %d x 48 B = %.1f MB' % (name, r['rounds'], r['n_boundary'], r['rounds'] * r['n_boundary'] * 48 / 1e6) for name, r in out.items()) +
              '; the stage also holds two scans, a sort of B keys and the host read.', '',
              '**Byte model of the successor and fill kernels.**  Successor: 12 B per boundary half-edge and (9 + 3 x %d) B per step of either walk.' % next(iter(out.values()))['index_bytes'],
              'Fill: 16 B per boundary half-edge, and per kept one 13 B in and one face and its loop (3 x %d + 4 B) out.  The repeated runs find' % next(iter(out.values()))['index_bytes'],
              'their inputs in the caches, so the rates are cache rates, not HBM rates; at these sizes the stages are a launch or two long.', '',
              '| mesh | walk steps (both ways) | successor bytes | successor ms | GB/s | fill bytes | fill faces ms | GB/s |', '|---|---|---|---|---|---|---|---|']
    for name, r in out.items():
        lines.append('| %s | %d | %d | %.3f | %.0f | %d | %.3f | %.0f |' % (
            name, r['walk_steps'], r['successor_model_bytes'], r['gpu_ms']['successor'], r['successor_model_bytes'] / max(r['gpu_ms']['successor'], 1e-9) / 1e6,
            r['fill_model_bytes'], r['gpu_ms']['fill faces'], r['fill_model_bytes'] / max(r['gpu_ms']['fill faces'], 1e-9) / 1e6))
    if any('host_ms' in r for r in out.values()):
        lines += ['', '| mesh | host copy | edge table | successor | rank | measures | fill | agrees with the GPU |', '|---|---|---|---|---|---|---|---|']
        for name, r in out.items():
            if 'host_ms' in r:
                lines.append('| %s | ' % name + ' | '.join('%.0f' % r['host_ms'][k] for k in ('copy', 'edge_table', 'successor', 'rank', 'measures', 'fill')) +
                             ' | %s |' % ('yes' if r['host_agrees'] else 'NO'))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the tables as markdown')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy timing')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mesh, _ = case_mesh(dev)
    out = {}
    for name, (v, f) in (('as meshed', (mesh.v, mesh.f)), ('less every 50th star', less_every_nth_star(mesh, 50))):
        b = mb.MeshBoundary(v, f)
        keep = b.loops().select(max_edges=MAX_EDGES, simple_only=False)
        stages(b, keep)                                                 # warm-up
        got = [stages(b, keep) for _ in range(args.reps)]
        r = got[0][1]
        new_faces = int(r.loop_edges[keep].sum().item())
        t = b.topology
        ib = f.element_size()
        rec = {'vertices': b.n_vertices, 'faces': b.n_faces, 'edges': int(t.num_edges), 'reps': args.reps, 'index_bytes': ib, 'n_boundary': r.n_boundary,
               'n_loops': r.n_loops, 'closed_loops': int(r.loop_closed.sum().item()), 'simple_loops': int(r.loop_simple.sum().item()),
               'kept_loops': int(keep.sum().item()), 'new_faces': new_faces, 'rounds': r.rounds, 'total_length': float(r.loop_length.sum().item()),
               'gpu_ms': {k: float(np.median([g[0][k] for g in got])) for k in got[0][0]}, 'topology_ms': topology_ms(v, f, min(args.reps, 5))}
        rec['gpu_ms']['total'] = sum(rec['gpu_ms'].values())
        # an interior edge at a border vertex is crossed once by the walk about the head that passes it and once by the one about the tail
        at_border = torch.zeros(b.n_vertices, dtype=torch.bool, device=dev)
        at_border[r.tail.long()] = True
        interior = t.edges[t.edge_classes == TOPO_INTERIOR].long()
        rec['walk_steps'] = 2 * int(at_border[interior].sum().item())
        rec['successor_model_bytes'] = 12 * r.n_boundary + (9 + 3 * ib) * rec['walk_steps']
        rec['fill_model_bytes'] = 16 * r.n_boundary + new_faces * (13 + 3 * ib + 4)
        if not args.no_host:
            torch.cuda.synchronize()
            rec['host_ms'], rec['host_info'] = host_path(v, f)
            rec['host_agrees'] = all(rec['host_info'][k] == rec[k] for k in ('n_boundary', 'n_loops', 'closed_loops', 'kept_loops', 'new_faces'))
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
