"""Per-chunk payloads (rank exchange, save_field): a chunk's voxels, features and solution as (int64 tensor, float32 tensor)."""
import numpy as np
import torch

from .. import ops
from .._lib import call, ptr, stream
from ..fields.kernel_field import KernelField
from ..fields.mask_fields import LayerField, NeuralField
from ..svh import SparseFeatureHierarchy


def _udf_levels(f):
    m = f.mask_field
    if not isinstance(m, NeuralField):
        return 0
    n = 0
    while n < f.svh.depth and n < len(m.features) and m.features[n] is not None:
        n += 1
    return n


def _pack(svh, kdim, approx, feat, alpha, udf_feats, level_set, ranges, band, shift):
    """Payload of the voxels ``ranges[d] = (lo, hi)`` of a hierarchy (one chunk of a batch, or a whole field)."""
    depth = svh.depth
    nu = len(udf_feats)
    off = svh.offsets
    sels, ns = [], []
    for d in range(depth):
        g = svh.level(d)
        lo, hi = ranges[d]
        if band is None:
            sels.append(slice(lo, hi))
            ns.append(hi - lo)
            continue
        w = g.voxel_size
        m = torch.zeros(hi - lo, dtype=torch.bool, device=svh.device)
        for a, blo, bhi in band:
            ca = (g.ijk[lo:hi, a].to(torch.float32) + 0.5) * w - float(shift[a])
            m |= (ca >= blo - 2.5 * w) & (ca <= bhi + 2.5 * w)
        idx = torch.nonzero(m).reshape(-1) + lo
        sels.append(idx)
        ns.append(int(idx.numel()))
    head = [depth, kdim, int(approx), nu] + ns
    ints = torch.cat([torch.tensor(head, dtype=torch.int64, device=svh.device)] + [svh.level(d).keys[sels[d]] for d in range(depth)])
    parts = [feat[d][sels[d]].reshape(-1) for d in range(depth)]
    for d in range(depth):
        s = sels[d]
        parts.append(alpha[off[d] + s.start:off[d] + s.stop] if isinstance(s, slice) else alpha[s + off[d]])
    if nu:
        parts += [udf_feats[d][sels[d]].reshape(-1) for d in range(nu)]
        parts.append(torch.tensor([level_set], dtype=torch.float32, device=svh.device))
    return ints, torch.cat(parts)


def pack_field(f, band=None, shift=None):
    """KernelField (+ its UDF mask features, when the mask is a NeuralField) -> (int64 tensor, float32 tensor).
    ``band`` (exchange_band, GLOBAL coordinates; ``shift`` = the translation of the field's frame, default the field's
    ``chunk_shift`` or 0): keep only the voxels that can contribute to an evaluation inside the band -- at level d those whose
    centre lies within 2.5 w_d of it (B-spline support 1.5 w_d, trilinear feature stencil 1 w_d).  This is the "halo" payload of
    the rank exchange: evaluations inside the band are bit-identical to those of the full field."""
    svh = f.svh
    nu = _udf_levels(f)
    if shift is None:
        shift = getattr(f, 'chunk_shift', (0.0, 0.0, 0.0))
    return _pack(svh, f.kdim, f.approx_kernel_grad, f._feat, f.alpha, [f.mask_field.features[d] for d in range(nu)],
                 f.mask_field.level_set if nu else 0.0, [(0, svh.num_voxels(d)) for d in range(svh.depth)], band, shift)


def _payload_heads(ints_list):
    """The headers (4 + at most 6 level counts) of several payloads in ONE host read."""
    if not ints_list:
        return []
    return torch.stack([torch.nn.functional.pad(i[:10], (0, 10 - min(10, int(i.numel())))) for i in ints_list]).tolist()


def _parse_payload(ints, flts, head=None):
    if head is None:
        head = _payload_heads([ints])[0]            # (was one host read per header entry)
    depth, kdim, approx, nu = int(head[0]), int(head[1]), bool(int(head[2])), int(head[3])
    ns = [int(v) for v in head[4:4 + depth]]
    off = 4 + depth
    keys = []
    for n in ns:
        keys.append(ints[off:off + n])
        off += n
    feats, fo = [], 0
    for n in ns:
        feats.append(flts[fo:fo + n * kdim].view(n, kdim))
        fo += n * kdim
    alphas = []
    for n in ns:
        alphas.append(flts[fo:fo + n])
        fo += n
    uf, level_set = [], 0.0
    if nu:
        for d in range(nu):
            uf.append(flts[fo:fo + ns[d] * 8].view(ns[d], 8))
            fo += ns[d] * 8
        level_set = float(flts[fo])
    return dict(depth=depth, kdim=kdim, approx=approx, nu=nu, ns=ns, keys=keys, feats=feats, alphas=alphas, udf=uf, level_set=level_set)


def fields_from_payloads(payloads, voxel_size, interpolators, device):
    """ONE KernelField from the payloads of several chunks -- [(key_lo of the chunk's slot, ints, flts), ...]; the slots are
    disjoint key ranges, so concatenating the chunks in slot order gives every level in canonical (ascending key) order."""
    payloads = [(k, i.to(device), f.to(device)) for k, i, f in sorted(payloads, key=lambda p: p[0])]
    heads = _payload_heads([i for _, i, _ in payloads])
    ps = [_parse_payload(i, f, h) for (_, i, f), h in zip(payloads, heads)]
    depth, kdim, approx, nu = ps[0]['depth'], ps[0]['kdim'], ps[0]['approx'], max(p['nu'] for p in ps)
    keys = [torch.cat([p['keys'][d] for p in ps]).contiguous() for d in range(depth)]
    svh = SparseFeatureHierarchy(voxel_size, depth, device).build_from_keys(keys, sorted_unique=True)
    feats = [torch.cat([p['feats'][d] for p in ps]).contiguous() for d in range(depth)]
    fld = KernelField(svh, interpolators, feats, approx_kernel_grad=approx)
    fld.alpha = torch.cat([p['alphas'][d] for d in range(depth) for p in ps]).contiguous()
    if nu:
        from ..nn.network import UDFDecoder
        uf = [None] * depth
        for d in range(nu):
            uf[d] = torch.cat([p['udf'][d] if d < p['nu'] else torch.zeros((p['ns'][d], 8), device=device) for p in ps]).contiguous()
        mask = NeuralField(svh, UDFDecoder(), uf)
        mask.set_level_set(next(p['level_set'] for p in ps if p['nu']))
        fld.set_mask_field(mask)
    return fld


def unpack_field(ints, flts, voxel_size, interpolators, device):
    return fields_from_payloads([(0, ints, flts)], voxel_size, interpolators, device)


class ChunkPart:
    """A KernelField in the exploded frame holding the chunks ``ids`` (ascending slot key), whole or as halos."""

    def __init__(self, field, ids, frame, solved=True):
        self.field, self.ids, self.frame, self.solved = field, list(ids), frame, solved
        self._ranges = None

    def ranges(self):
        """{chunk: [(lo, hi) per level]} voxel index ranges (one host read)."""
        if self._ranges is None:
            svh = self.field.svh
            kr = [self.frame.key_range(c) for c in self.ids]
            klo = torch.tensor([k[0] for k in kr], dtype=torch.int64, device=svh.device)
            khi = torch.tensor([k[1] for k in kr], dtype=torch.int64, device=svh.device)
            lo = torch.stack([torch.searchsorted(svh.level(d).keys, klo >> (3 * d)) for d in range(svh.depth)], 1).tolist()
            hi = torch.stack([torch.searchsorted(svh.level(d).keys, khi >> (3 * d)) for d in range(svh.depth)], 1).tolist()
            self._ranges = {c: [(lo[i][d], hi[i][d]) for d in range(svh.depth)] for i, c in enumerate(self.ids)}
        return self._ranges

    def pack_chunk(self, c, band=None):
        f = self.field
        nu = _udf_levels(f)
        return _pack(f.svh, f.kdim, f.approx_kernel_grad, f._feat, f.alpha, [f.mask_field.features[d] for d in range(nu)],
                     f.mask_field.level_set if nu else 0.0, self.ranges()[c], band, self.frame.shift(c))

    def pack_halos(self, bands):
        """``{c: (ints, flts)}`` for every chunk of the part -- exactly what ``pack_chunk(c, bands[c])`` returns, made for all chunks at
        once: one mask and one compaction per LEVEL instead of one per chunk and level (8 chunks x 5 levels of small launches and
        host syncs were 11 ms of a rank's 80 ms at 8 ranks, tools/prof_rank_tail.py)."""
        f = self.field
        svh, dev, depth = f.svh, f.svh.device, f.svh.depth
        nu = _udf_levels(f)
        ids, nc = self.ids, len(self.ids)
        if nc == 0:
            return {}
        kr = [self.frame.key_range(c) for c in ids]
        klo = torch.tensor([k[0] for k in kr], dtype=torch.int64, device=dev)
        shift = torch.from_numpy(np.stack([np.asarray(self.frame.shift(c), np.float32) for c in ids])).to(dev)      # [nc, 3]
        # band table: up to two intervals per axis (the faces shared with the chunk before / after); none = an empty interval
        blo = np.full((nc, 3, 2), np.inf)
        bhi = np.full((nc, 3, 2), -np.inf)
        for i, c in enumerate(ids):
            used = [0, 0, 0]
            for a, lo_, hi_ in bands[c]:
                blo[i, a, used[a]], bhi[i, a, used[a]] = lo_, hi_
                used[a] += 1
        off = svh.offsets
        sel, cnt = [], []
        for d in range(depth):
            g = svh.level(d)
            if g.num_voxels == 0:
                sel.append(torch.zeros(0, dtype=torch.long, device=dev))
                cnt.append(torch.zeros(nc, dtype=torch.long, device=dev))
                continue
            w = g.voxel_size
            # (thresholds in double, compared in fp32, as pack_field does with Python scalars; csrc/chunks.hip k_halo_band_flags)
            tlo = torch.from_numpy((blo - 2.5 * w).astype(np.float32)).to(dev)
            thi = torch.from_numpy((bhi + 2.5 * w).astype(np.float32)).to(dev)
            seg = torch.empty(g.num_voxels, dtype=torch.int32, device=dev)
            flags = torch.empty(g.num_voxels, dtype=torch.int32, device=dev)
            call('nksr_halo_band_flags', ptr(g.keys), ptr(g.ijk), g.num_voxels, ptr((klo >> (3 * d)).contiguous()), nc, ptr(shift), ptr(tlo), ptr(thi),
                 float(w), ptr(seg), ptr(flags), stream())
            idx = ops.compact(flags).long()
            sel.append(idx)
            cnt.append(torch.bincount(seg[idx].long(), minlength=nc))
        counts = torch.stack(cnt, 1).tolist()                                   # [nc][depth]   (one host read)
        keys = [svh.level(d).keys[sel[d]] for d in range(depth)]
        feats = [f._feat[d][sel[d]] for d in range(depth)]
        alphas = [f.alpha[sel[d] + off[d]] for d in range(depth)]
        udf = [f.mask_field.features[d][sel[d]] for d in range(nu)]
        heads = torch.tensor([[depth, f.kdim, int(f.approx_kernel_grad), nu] + counts[i] for i in range(nc)], dtype=torch.int64, device=dev)
        tail = [torch.tensor([f.mask_field.level_set], dtype=torch.float32, device=dev)] if nu else []
        out, o = {}, [0] * depth
        for i, c in enumerate(ids):
            sl = [slice(o[d], o[d] + counts[i][d]) for d in range(depth)]
            ints = torch.cat([heads[i]] + [keys[d][sl[d]] for d in range(depth)])
            parts = [feats[d][sl[d]].reshape(-1) for d in range(depth)] + [alphas[d][sl[d]] for d in range(depth)]
            parts += [udf[d][sl[d]].reshape(-1) for d in range(nu)] + tail
            out[c] = (ints, torch.cat(parts))
            o = [o[d] + counts[i][d] for d in range(depth)]
        return out

    def chunk_view(self, c, interpolators):
        """Chunk c as a KernelField of its own (exploded frame): tests, save_field, simulated ranks."""
        ints, flts = self.pack_chunk(c)
        g = unpack_field(ints, flts, self.field.svh.voxel_size, interpolators, self.field.device)
        g.chunk_shift = tuple(float(v) for v in self.frame.shift(c))
        if g.mask_field is None:
            g.set_mask_field(LayerField(g.svh, getattr(self.field.mask_field, 'adaptive_depth', 1)))
        g.meshing_depth = getattr(self.field, 'meshing_depth', 1)
        info = self.field.solve_info
        g.solve_info = {}
        if self.solved and info:
            si = info.get('segment_info')
            i = self.ids.index(c)
            g.solve_info = {'M': int(g.svh.num_unknowns), 'nnz': 0, 'fused': True,
                            'iters': int(si[i, 0]) if si is not None else info.get('iters'),
                            'rel_residual': float(si[i, 1]) if si is not None else info.get('rel_residual')}
        return g
