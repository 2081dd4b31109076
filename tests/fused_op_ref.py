"""Plain numpy / scipy restatement of the matrix-free operator (csrc/fused_tables.hip, fused_sweep.hip, fused.hip; nksr_fused_op_t) and the crafted row layouts
its sweep is tested on (tests/test_fused_op_ref_cpu.py, tests/test_gpu_fused_operator.py).

The operator is completely defined by its arrays:

    y = R^T (R x) + reg x,      R[r, nbr_d[row_cells[d][r]][s]] = rows_all[d][r][s]

(row r, level d, stencil slot s; a slot whose cell or neighbour is absent belongs to no unknown).  Everything else -- units,
items, workgroups, partial blocks, the slot-major tables -- is bookkeeping of HOW the HIP kernels walk the rows; tables_ref
restates that bookkeeping from the header comment of nksr_fused_op_t (include/nksr_hip.h) with loops over rows, not with the
kernels' arithmetic.
"""
import numpy as np
import scipy.sparse as sp

ITEM_ROWS = 32          # rows of a work item (FZ_RC)
WG_ITEMS = 8            # items of a workgroup (FZ_HW)
WG_ROWS = ITEM_ROWS * WG_ITEMS
STAGE0, STAGE1 = 96, 32  # staged level-0 / level-1 cells of a workgroup (FZ_STAGE0 / FZ_STAGE1)
RCAP = 288              # rows of a workgroup whose factor records are staged (FZ_RCAP)
BIG = 16                # a cell with more partial blocks gets a workgroup of its own in the per-cell sum
GROUP = 4               # cells a half-wave sums together otherwise (FZ_GI)
VOXEL = 0.1
_BIAS = 1 << 20


# ---- integer conventions, restated -------------------------------------------------------------------------
def site_ijk0(xyz, voxel_size=VOXEL):
    """Level-0 cell of every site: floor(x * inv_w0), the product in fp32."""
    p = np.asarray(xyz, np.float32) * np.float32(1.0 / float(voxel_size))
    return np.floor(p).astype(np.int64)


def _spread(v):
    out = np.zeros(v.shape, np.int64)
    for b in range(21):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def morton(ijk):
    """Morton key of level-0 integer coordinates (x = lowest bit), biased as the library's keys are."""
    b = np.asarray(ijk, np.int64) + _BIAS
    return _spread(b[..., 0]) | (_spread(b[..., 1]) << 1) | (_spread(b[..., 2]) << 2)


def morton_decode(code):
    """Integer coordinates (unbiased) of the codes 0, 1, 2, ... of a Morton-aligned cube at the origin."""
    code = np.asarray(code, np.int64)
    out = np.zeros(code.shape + (3,), np.int64)
    for b in range(21):
        for a in range(3):
            out[..., a] |= ((code >> (3 * b + a)) & 1) << b
    return out


def _pack(ijk):
    v = np.asarray(ijk, np.int64) + _BIAS
    return (v[..., 0] << 42) | (v[..., 1] << 21) | v[..., 2]


def _lookup(level_ijk, query_ijk):
    """index of query_ijk in level_ijk, -1 where absent"""
    have = _pack(level_ijk)
    order = np.argsort(have, kind='stable')
    q = _pack(query_ijk)
    if have.size == 0:
        return np.full(q.shape, -1, np.int64)
    pos = np.minimum(np.searchsorted(have[order], q), have.size - 1)
    return np.where(have[order][pos] == q, order[pos], -1)


def level_offsets(levels):
    n = [int(np.asarray(L.ijk).shape[0]) for L in levels]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def nbr_global_ref(levels):
    """[M, 27] global unknown index of every neighbour voxel (slot s = (dx + 1) 9 + (dy + 1) 3 + dz + 1), -1 where absent."""
    off = level_offsets(levels)
    out = []
    for d, L in enumerate(levels):
        ijk = np.asarray(L.ijk, np.int64)
        nb = np.empty((ijk.shape[0], 27), np.int64)
        s = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    j = _lookup(ijk, ijk + np.array([dx, dy, dz]))
                    nb[:, s] = np.where(j >= 0, j + off[d], -1)
                    s += 1
        out.append(nb)
    return np.concatenate(out)


def row_cells_ref(levels, sites, rows_per_site, voxel_size=VOXEL, segment_key_lo=None, with_sets=False):
    """row_cells [depth, rows_total] of the ONE Morton-ordered row list of the site sets ``sites`` (list of [n, 3] arrays; set i owns
    rows_per_site[i] rows per site): the stable merge by level-0 Morton key, earlier sets first on equal keys.  The cell of a site
    at level d is floor(x inv_w0) >> d, looked up in the level's ijk: its GLOBAL unknown index, -1 where the cell is absent.
    ``segment_key_lo`` (sorted level-0 keys): the rows of every segment are padded to a multiple of 256 with rows that have no cell.
    ``with_sets``: also the site set of every row (-1: a pad row)."""
    off = level_offsets(levels)
    ijk0 = np.concatenate([site_ijk0(x, voxel_size) for x in sites])
    which = np.concatenate([np.full(len(x), i, np.int64) for i, x in enumerate(sites)])
    nrow = np.asarray(rows_per_site, np.int64)[which]
    key = morton(ijk0)
    order = np.lexsort((which, key))                         # by key, then by set; stable inside a set
    ijk0, which, nrow, key = ijk0[order], which[order], nrow[order], key[order]
    first = np.cumsum(nrow) - nrow
    rows_total = int(nrow.sum())
    if segment_key_lo is not None:
        klo = np.asarray(segment_key_lo, np.int64)
        seg = np.searchsorted(klo, key, side='right') - 1
        assert (seg >= 0).all(), 'a site lies before the first segment'
        rows_seg = np.bincount(seg, weights=nrow, minlength=len(klo)).astype(np.int64)
        pad = (-rows_seg) % WG_ROWS
        first = first + (np.cumsum(pad) - pad)[seg]
        rows_total += int(pad.sum())
    cells = np.full((len(levels), rows_total), -1, np.int64)
    sets = np.full(rows_total, -1, np.int64)
    site_rows = np.repeat(first, nrow) + (np.arange(int(nrow.sum())) - np.repeat(np.cumsum(nrow) - nrow, nrow))
    sets[site_rows] = np.repeat(which, nrow)
    for d, L in enumerate(levels):
        c = _lookup(np.asarray(L.ijk, np.int64), ijk0 >> d)
        cells[d, site_rows] = np.repeat(np.where(c >= 0, c + off[d], -1), nrow)
    cells = cells.astype(np.int32)
    return (cells, sets) if with_sets else cells


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
def unit_starts(row_cells):
    """bool [rows_total]: row r starts a unit (a maximal run of rows in the same cell at every level)"""
    rc = np.asarray(row_cells)
    st = np.ones(rc.shape[1], bool)
    st[1:] = (rc[:, 1:] != rc[:, :-1]).any(0)
    return st


def item_entries(rows_total):
    nitems = (rows_total + ITEM_ROWS - 1) // ITEM_ROWS
    nwg = (nitems + WG_ITEMS - 1) // WG_ITEMS
    return nitems, nwg, nwg * WG_ITEMS + 1


def item_begin_ref(row_cells):
    rc = np.asarray(row_cells)
    rows_total = rc.shape[1]
    nitems, nwg, nent = item_entries(rows_total)
    starts = np.nonzero(unit_starts(rc))[0] if rows_total else np.zeros(0, np.int64)
    ib = np.full(nent, rows_total, np.int64)
    for i in range(nitems):
        k = np.searchsorted(starts, i * ITEM_ROWS)          # first unit start >= 32 i
        if k < len(starts):
            ib[i] = starts[k]
    return ib


def wg_of(item_begin, nwg, r):
    """workgroup of row r: the last w with item_begin[8 w] <= r"""
    heads = np.asarray(item_begin)[0:nwg * WG_ITEMS:WG_ITEMS]
    return np.maximum(np.searchsorted(heads, r, side='right') - 1, 0)


def tables_ref(row_cells, M, depth, nbr_global=None):
    """The operator's tables from row_cells alone (+ the neighbour table for nbr32 / nbrT): span [3, M], item_begin, counts
    [M + 1], offsets [M + 1], nblocks, multi, n_multi, n_big, nbr32 [M, 32], nbrT [27, M]."""
    rc = np.asarray(row_cells).reshape(depth, -1)
    rows_total = rc.shape[1]
    nitems, nwg, nent = item_entries(rows_total)
    first = np.full(M, -1, np.int64)
    last = np.full(M, -1, np.int64)
    for d in range(depth):
        for r in range(rows_total):                          # (plain loop: the definition)
            c = rc[d, r]
            if c >= 0:
                if first[c] < 0:
                    first[c] = r
                last[c] = r
    ib = item_begin_ref(rc)
    wgfirst = np.zeros(M, np.int64)
    counts = np.zeros(M + 1, np.int64)
    has = first >= 0
    if nwg > 0 and has.any():
        w0, w1 = wg_of(ib, nwg, first[has]), wg_of(ib, nwg, last[has])
        wgfirst[has] = w0
        n = w1 - w0 + 1
        counts[:M][has] = np.where(n == 1, 0, n)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]])
    big = np.nonzero(counts[:M] > BIG)[0]
    multi = np.concatenate([big, np.nonzero((counts[:M] > 1) & (counts[:M] <= BIG))[0]])
    T = {'span': np.stack([first, last, wgfirst]).astype(np.int32), 'item_begin': ib.astype(np.int32), 'counts': counts.astype(np.int32),
         'offsets': offsets.astype(np.int32), 'nblocks': int(counts.sum()), 'multi': multi.astype(np.int32), 'n_multi': int(multi.size),
         'n_big': int(big.size), 'nwg': nwg, 'nitems': nitems}
    if nbr_global is not None:
        nb = np.asarray(nbr_global)
        nbr32 = np.zeros((M, 32), np.int64)
        nbr32[:, :27] = nb
        nbr32[:, 27] = offsets[:M] - wgfirst
        nbr32[:, 28], nbr32[:, 29] = first, last
        T['nbr32'] = nbr32.astype(np.int32)
        T['nbrT'] = np.ascontiguousarray(nb.T).astype(np.int32)
    return T


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
def valid_slots(row_cells, nbr_global):
    """bool [depth, rows_total, 27]: the slot belongs to an unknown (the row has a cell at that level and the cell that neighbour)"""
    rc = np.asarray(row_cells)
    nb = np.asarray(nbr_global)
    return (rc >= 0)[:, :, None] & (nb[np.maximum(rc, 0)] >= 0)


def rows_matrix(rows, row_cells, nbr_global, M):
    """R as a scipy CSR [rows_total, M]: int64 when the rows are integral, fp64 otherwise."""
    rows = np.asarray(rows)
    rc = np.asarray(row_cells)
    depth, R = rc.shape
    rows = rows.reshape(depth, R, 27)
    integral = np.issubdtype(rows.dtype, np.integer) or bool((rows == np.rint(rows)).all())
    dt = np.int64 if integral else np.float64
    ok = valid_slots(rc, nbr_global)
    cols = np.asarray(nbr_global)[np.maximum(rc, 0)]                      # [depth, R, 27]
    rr = np.broadcast_to(np.arange(R)[None, :, None], ok.shape)
    A = sp.coo_matrix((rows[ok].astype(dt), (rr[ok], cols[ok])), shape=(R, M)).tocsr()      # (duplicates add: none occur, a row's 27 D columns differ)
    return A


def _integral(a):
    a = np.asarray(a)
    return np.issubdtype(a.dtype, np.integer) or bool((a == np.rint(a)).all())


def operator_ref(rows, row_cells, nbr_global, targets, x, reg, Rm=None):
    """y = R^T (R x) + reg x, b = R^T t, diag = reg + sum R^2, nnz = the non-zero slots of the rows, and the magnitudes
    mag = |R|^T |R| |x| + reg |x| and mag_b = |R|^T |t| that scale the rounding error of one fp32 evaluation.
    int64 when every input is integral (reg included, or 2 reg: then y and diag come back DOUBLED -- see 'scale'), fp64 otherwise."""
    M = np.asarray(nbr_global).shape[0]
    Rm = rows_matrix(rows, row_cells, nbr_global, M) if Rm is None else Rm
    x, t = np.asarray(x), np.asarray(targets)
    scale = 1
    if Rm.dtype == np.int64 and _integral(x) and _integral(t) and (_integral(reg) or _integral(2 * reg)):
        scale = 1 if _integral(reg) else 2                  # reg = 0.5: everything times two stays integral
        x, t, r = np.rint(x).astype(np.int64), np.rint(t).astype(np.int64), int(round(scale * reg))
    else:
        Rm, x, t, r = Rm.astype(np.float64), x.astype(np.float64), t.astype(np.float64), float(reg)
    Ra = abs(Rm)
    out = {'y': scale * (Rm.T @ (Rm @ x)) + r * x, 'b': Rm.T @ t, 'diag': r + scale * np.asarray(Rm.multiply(Rm).sum(0)).reshape(-1),
           'nnz': int(np.count_nonzero(np.asarray(rows))), 'scale': scale,
           'mag': (Ra.T @ (Ra @ np.abs(x))) + (r / scale) * np.abs(x), 'mag_b': Ra.T @ np.abs(t)}
    return out


def rounding_steps(T, nbr_global, depth):
    """m_j of the bound |y - y_ref|_j <= gamma(m_j) mag_j: every product of the sum y_j passes through at most 27 depth additions
    (t), the chain over the rows of its cell (the largest row count among j's 27 neighbour cells), that cell's partial blocks,
    and 27 + 8 additions of the gather and the workgroup exchange."""
    first, last = T['span'][0].astype(np.int64), T['span'][1].astype(np.int64)
    nrows = np.where(first >= 0, last - first + 1, 0)
    nb = np.asarray(nbr_global)
    nr = np.where(nb >= 0, nrows[np.maximum(nb, 0)], -1)
    best = np.argmax(nr, 1)
    cell = nb[np.arange(nb.shape[0]), best]
    m = 27 * depth + np.maximum(nr.max(1), 0) + np.where(cell >= 0, T['counts'][np.maximum(cell, 0)], 0) + 27 + 8
    return m.astype(np.float64)


def gamma(m, u=2.0 ** -24):
    m = np.asarray(m, np.float64)
    return m * u / (1.0 - m * u)


def integer_case(row_cells, nbr_global, seed, dense_limit=4000):
    """Integer rows, targets and three x for the bit-for-bit comparison.  Rows from {-1, 0, 1}; a slot stays zero wherever the row
    kernels write zero (absent cell, absent neighbour, pad row).  Every partial sum must stay below 2^24 (the CPU test asserts
    mag.max() < 2^24): row lists of up to ``dense_limit`` rows get all 27 slots and |x|, |t| <= 3 (mag <= rows x 27 depth x 3);
    longer ones two +-1 slots per row and level and |x| <= 1 (mag <= rows x 2 depth)."""
    rc = np.asarray(row_cells)
    depth, R = rc.shape
    M = np.asarray(nbr_global).shape[0]
    rs = np.random.RandomState(seed)
    big = R > dense_limit
    if big:
        rows = np.zeros((depth, R, 27), np.int64)
        for k in range(2):
            s = rs.randint(0, 27, (depth, R))
            np.put_along_axis(rows, s[:, :, None], rs.choice([-1, 1], (depth, R, 1)), 2)
    else:
        rows = rs.randint(-1, 2, (depth, R, 27)).astype(np.int64)
    rows[~valid_slots(rc, nbr_global)] = 0
    amp = 1 if big else 3
    t = rs.randint(-3, 4, R).astype(np.int64)
    t[(rc < 0).all(0)] = 0
    xs = [rs.randint(-amp, amp + 1, M).astype(np.int64) for _ in range(3)]
    return rows, t, xs


def compare_exact(name, got, ref):
    """The CPU-side comparison helper of the bit-for-bit cases: ``got`` (what the GPU returned, fp32) against the int64 reference."""
    g = np.asarray(got)
    assert g.shape == np.asarray(ref).shape, '%s: shape %s vs %s' % (name, g.shape, np.asarray(ref).shape)
    bad = np.nonzero(g.astype(np.float64) != np.asarray(ref).astype(np.float64))[0]
    assert bad.size == 0, '%s: %d of %d entries differ; first at %d: %r vs %r' % (name, bad.size, g.size, bad[0], g[bad[0]], np.asarray(ref)[bad[0]])


# ---- what a layout looks like to the sweep ----------------------------------------------------------------------------------------------
def layout_stats(row_cells, row_sets=None, T=None, M=None):
    """The properties of a row list the sweep's branches depend on (derived from row_cells with loops, independent of tables_ref
    except for item_begin / counts, which it takes from ``T`` or recomputes)."""
    rc = np.asarray(row_cells)
    depth, R = rc.shape
    if T is None:
        T = tables_ref(rc, int(rc.max()) + 1 if M is None else M, depth)
    ib, nwg, nitems = T['item_begin'].astype(np.int64), T['nwg'], T['nitems']
    st = unit_starts(rc)
    ustart = np.nonzero(st)[0]
    ulen = np.diff(np.concatenate([ustart, [R]]))
    S = {'rows_total': R, 'nwg': nwg, 'max_unit': int(ulen.max()) if R else 0, 'units': int(ustart.size)}
    S['units_longer_than'] = {n: int((ulen > n).sum()) for n in (ITEM_ROWS, WG_ROWS, RCAP)}
    S['empty_items'] = int(sum(ib[i] == ib[i + 1] for i in range(nitems)))
    S['empty_wgs'] = int(sum(ib[8 * w] == ib[8 * w + 8] for w in range(nwg)))
    S['max_wg_rows'] = int(max([ib[8 * w + 8] - ib[8 * w] for w in range(nwg)] or [0]))
    S['max_wg_cells0'] = S['max_wg_cells1'] = 0
    S['wg_beyond_stage0'] = S['wg_beyond_stage1'] = S['wg_first_row_without_c0'] = 0
    for w in range(nwg):
        a, b = ib[8 * w], ib[8 * w + 8]
        if a >= b:
            continue
        for d, cap, key in ((0, STAGE0, '0'), (1, STAGE1, '1')):
            if d >= depth:
                continue
            c = np.unique(rc[d, a:b])
            c = c[c >= 0]
            S['max_wg_cells' + key] = max(S['max_wg_cells' + key], int(c.size))
            if rc[d, a] >= 0 and c.size and (c - rc[d, a] >= cap).any():
                S['wg_beyond_stage' + key] += 1
        S['wg_first_row_without_c0'] += int(rc[0, a] < 0)
    # coarse cells whose pieces inside ONE workgroup lie in items with an empty item between them
    gap = 0
    for w in range(nwg):
        items = [(ib[i], ib[i + 1]) for i in range(8 * w, 8 * w + 8)]
        for d in range(1, depth):
            seen = {}
            for h, (a, b) in enumerate(items):
                for c in np.unique(rc[d, a:b]) if b > a else []:
                    if c >= 0:
                        seen.setdefault(int(c), []).append(h)
            for c, hs in seen.items():
                for h0, h1 in zip(hs[:-1], hs[1:]):
                    if h1 - h0 > 1 and all(items[h][0] == items[h][1] for h in range(h0 + 1, h1)):
                        gap += 1
    S['exchange_over_empty_item'] = gap
    present = rc >= 0
    fp = np.where(present.any(0), present.argmax(0), -1)
    S['first_present'] = sorted(set(int(v) for v in fp))
    S['rows_without_cell'] = int((~present.any(0)).sum())
    nocell = np.nonzero(~present.any(0))[0]
    S['runs_without_cell'] = int((np.diff(nocell) > 1).sum() + 1) if nocell.size else 0
    if row_sets is not None:
        rs_ = np.asarray(row_sets)
        uid = np.cumsum(st) - 1
        has0 = np.zeros(ustart.size, bool)
        has1 = np.zeros(ustart.size, bool)
        has0[uid[rs_ == 0]] = True
        has1[uid[rs_ == 1]] = True
        S['units_with_both_sets'] = int((has0 & has1).sum())
    cnt = T['counts'][:-1]
    S['counts'] = sorted(set(int(v) for v in cnt if v > 0))
    S['cells_2_to_16'] = int(((cnt > 1) & (cnt <= BIG)).sum())
    return S


# ---- crafted clouds ---------------------------------------------------------------------------------------------------------------------
_R3 = np.array([0.8191725133961645, 0.6710436067037893, 0.5497004779019703])      # the plastic-number sequence: distinct, well spread


def voxel_points(codes, counts, origin=(0, 0, 0)):
    """``counts[i]`` points inside the level-0 voxel with Morton code ``codes[i]`` of the cube at ``origin`` (voxel units), fp32,
    kept away from the voxel's faces."""
    codes, counts = np.asarray(codes, np.int64), np.asarray(counts, np.int64)
    vox = np.repeat(morton_decode(codes) + np.asarray(origin, np.int64), counts, 0)
    k = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
    frac = 0.125 + 0.75 * (((k[:, None] + 1) * _R3[None] + np.repeat(codes, counts)[:, None] * 0.318) % 1.0)
    return ((vox + frac) * VOXEL).astype(np.float32)


class Layout:
    """cloud: the points the hierarchy is built from (build_point_neighborhood); pos / nrm: the position / normal sites (None: no
    such set); nrm may be a callable of the oracle hierarchy (sites taken from the hierarchy's own voxel centres)."""

    def __init__(self, name, cloud, pos, nrm, depth=4, segments=False):
        self.name, self.cloud, self.pos, self._nrm, self.depth, self.segments = name, cloud, pos, nrm, depth, segments

    def normal_sites(self, oh):
        return self._nrm(oh) if callable(self._nrm) else self._nrm

    def site_sets(self, oh, rows_per_normal=3):
        nrm = self.normal_sites(oh)
        sets = [(x, r) for x, r in ((self.pos, 1), (nrm, rows_per_normal)) if x is not None and len(x)]
        return [s[0] for s in sets], [s[1] for s in sets]

    def segment_key_lo(self, oh):
        """two segments cut from the sorted coarsest-level keys, as test_row_order_by_rank_passes_equals_the_sorted_merge cuts them"""
        if not self.segments:
            return None
        k = np.asarray(oh.levels[-1].keys, np.int64)
        return np.array([k[0], k[len(k) // 2]], np.int64) << (3 * (self.depth - 1))


def _centres(oh, d):
    return np.asarray(oh.levels[d].centers(), np.float32)


def _mixed(name, depth=4, segments=False):
    cloud = voxel_points(np.arange(125), np.full(125, 3), origin=(12, 12, 12))      # across the faces of coarse cells of every level
    nrm = (lambda oh: np.concatenate([_centres(oh, 0), _centres(oh, 1)])) if depth > 1 else (lambda oh: _centres(oh, 0))
    return Layout(name, cloud, cloud, nrm, depth, segments)


def _clumps():
    counts = np.ones(512, np.int64)
    counts[28], counts[100], counts[200] = 40, 300, 700
    cloud = voxel_points(np.arange(512), counts)
    return Layout('clumps', cloud, cloud, None)


# points per voxel of the `blocks` layout, by Morton code (tree_depth 5: codes 0 .. 4095 share ONE level-4 cell).  Tuned with
# tables_ref: level-2 cells of 4096 rows that start on / half-way between workgroup boundaries (16 and 17 blocks), one of 7040 rows
# (28), level-3 cells of 15 360 / 31 232 / 19 456 rows (61, 122, 77 blocks), the level-4 cell with all 66 073 rows (259), level-1
# cells of a few hundred rows (2 .. 5).  No unit is longer than 110 rows: every workgroup of a cell's span holds rows of it.
def _blocks():
    counts = np.zeros(1536 + 8, np.int64)
    counts[0:64] = 64
    counts[64:66] = 64
    counts[128:192] = 64
    counts[192:256] = 110
    counts[512:1024] = 61
    counts[1024:1536] = 38
    counts[1536:1541] = 5
    codes = np.nonzero(counts)[0]
    cloud = voxel_points(codes, counts[codes])
    return Layout('blocks', cloud, cloud, None, depth=5)


def _absent():
    cloud = voxel_points(np.arange(64), np.full(64, 1), origin=(8, 8, 8))
    far = (cloud - np.float32(100 * VOXEL)).astype(np.float32)                      # outside every level; sorts before everything else
    pos = np.concatenate([cloud, far, far + np.float32(0.01)])
    return Layout('absent', cloud, pos, lambda oh: np.concatenate([_centres(oh, 1), _centres(oh, 2), far[:40]]))


def _sparse1():
    codes = np.arange(512) * 8                                                        # one voxel of every level-1 cell of a 16^3 cube
    cloud = voxel_points(codes, np.ones(512, np.int64))
    return Layout('sparse1', cloud, cloud, None)


TINY_ROWS = (1, 31, 32, 33, 255, 256, 257)


def _tiny(n):
    cloud = voxel_points(np.arange(n), np.ones(n, np.int64))
    return Layout('tiny%d' % n, cloud, cloud, None)


LAYOUTS = {'sparse1': _sparse1, 'clumps': _clumps, 'blocks': _blocks, 'absent': _absent, 'mixed': lambda: _mixed('mixed'),
           'segments2': lambda: _mixed('segments2', segments=True),
           'depth1': lambda: _mixed('depth1', 1), 'depth2': lambda: _mixed('depth2', 2), 'depth6': lambda: _mixed('depth6', 6)}
LAYOUTS.update({'tiny%d' % n: (lambda n=n: _tiny(n)) for n in TINY_ROWS})
FACTOR_LAYOUTS = ['clumps', 'mixed', 'absent', 'segments2'] + ['tiny%d' % n for n in TINY_ROWS]
_cache = {}


def layout(name):
    """the layout, its oracle hierarchy, neighbour table, reference row cells (dense row format), row sets and tables -- computed once"""
    if name not in _cache:
        from oracle import hierarchy
        lay = LAYOUTS[name]()
        oh = hierarchy.Hierarchy(VOXEL, lay.depth).build_point_neighborhood(lay.cloud)
        nb = nbr_global_ref(oh.levels)
        sites, rps = lay.site_sets(oh)
        rc, sets = row_cells_ref(oh.levels, sites, rps, segment_key_lo=lay.segment_key_lo(oh), with_sets=True)
        T = tables_ref(rc, nb.shape[0], lay.depth, nb)
        _cache[name] = {'layout': lay, 'oh': oh, 'nbr': nb, 'row_cells': rc, 'row_sets': sets, 'tables': T, 'M': nb.shape[0]}
    return _cache[name]
