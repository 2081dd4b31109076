"""numpy restatement of the coarse-level block preconditioner (csrc/cheb.hip, k_cheb_coeffs .. cheb_apply) and the inputs its tests
share.  Imports nothing of nksr_amd.

The operator (include/nksr_hip.h, nksr_coarse_precond_t).  With S = D^-1/2 A D^-1/2 = U diag(lam) U^T, k = steps, the interval
[lmax / ratio, lmax], theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2:

    z = D^-1/2 U p(lam) U^T D^-1/2 r,      p(l) = (1 - T_k((theta - l) / delta) / T_k(theta / delta)) / l

(the k-1 degree polynomial of the Chebyshev iteration from x0 = 0: its residual polynomial is the scaled T_k).  The kernels realise
it as the recurrence  d0 = r / D / theta;  k times { y += d; res -= A d; d = a_i d + b_i res / D };  z = y  -- apply_recurrence --
and, for the packed block, in the scaled variables res' = D^-1/2 res, d' = D^1/2 d on S_h, the half-rounded, dropped S that the packed
words denote (pack_ref returns it: half precision is then part of the operator, not of a tolerance).

A degenerate segment (lmax <= 0 or not finite) has the table {1, 0, 0, ...}: p = 1, z = r / D, one Jacobi step.

make_block: block-diagonal SPD test matrices A = B B^T + E per segment with a prescribed sparsity pattern.  Every off-diagonal pair
{i, j} is one column of B with the two entries b_ie, b_je, so A_ij = b_ie b_je (one product, mirrored: bitwise symmetric in fp32) and
A_ii = sum_e b_ie^2 + E_i.  With b_ie = w_e a_i, b_je = -w_e a_j on a chain-like graph, x_i = 1 / a_i is a near-null vector and the
smooth modes of the chain follow it: the Jacobi-scaled spectrum is wide (lmax / lmin ~ 1e3, many eigenvalues below lmax / ratio).
Rows listed as `weak` get a large E_i: all their scaled entries fall below the packer's drop tolerance."""
import functools

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest): no fp32 result is expected closer than this to the exact one
MAX_STEPS = 16            # NKSR_PC_MAX_STEPS
STRIDE = 1 + 2 * MAX_STEPS
HUB_DEGREES = (320, 0, 257, 256, 255, 65, 64, 63, 17, 16, 15, 1)      # off-diagonal row lengths the kernels' trip counts turn on


# ---- test matrices --------------------------------------------------------------------------------------------------------------
def make_block(row_seg, seed, hubs=(), weak_frac=0.1, reach=3, eps=5e-4):
    """row_seg [n] (any order: the segment of every row in PCG order).  Per segment: the ordinary rows form a chain, each joined to
    its `reach` successors, plus a few long-range pairs; the first len(hubs) rows (in PCG order) get exactly hubs[k] off-diagonal
    entries, towards a contiguous stretch of the chain (as a coarse basis function overlaps the finer ones under it); the row after
    them is `weak` with a few entries, and so is a tenth of the ordinary rows.  `hubs` applies to every segment large enough to hold
    them (3 x the largest degree), smaller segments get ordinary rows only.
    -> dict: rowptr, cols, vals (CSR, off-diagonal columns in random order, the diagonal LAST), diag, row_seg, nseg, dense (fp64 of the
    fp32 values)."""
    rng = np.random.default_rng(seed)
    row_seg = np.asarray(row_seg, np.int32)
    n = len(row_seg)
    nseg = int(row_seg.max()) + 1
    pair_i, pair_j = [], []
    weak = np.zeros(n, bool)
    for c in range(nseg):
        rows = np.nonzero(row_seg == c)[0]
        m = len(rows)
        nh = len(hubs) if hubs and m >= 3 * max(hubs) else 0
        ordinary = rows[nh + 1:] if nh else rows
        mo = len(ordinary)
        if nh:
            weak[rows[nh]] = True
            for k, deg in enumerate(tuple(hubs) + (5,)):                   # (the weak row after the hubs holds five entries)
                start = int(rng.integers(0, mo - deg + 1))
                pair_i += [rows[k]] * deg
                pair_j += ordinary[start:start + deg].tolist()
        if mo > 1:
            weak[ordinary[rng.random(mo) < weak_frac]] = True
            for o in range(1, min(reach, mo - 1) + 1):                     # the chain
                pair_i += ordinary[:mo - o].tolist()
                pair_j += ordinary[o:].tolist()
            far = mo // 64                                                 # and a few long-range pairs
            pair_i += rng.choice(ordinary, far).tolist()
            pair_j += rng.choice(ordinary, far).tolist()
    pi, pj = np.asarray(pair_i, np.int64), np.asarray(pair_j, np.int64)
    lo, hi = np.minimum(pi, pj), np.maximum(pi, pj)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])            # every pair once
    lo, hi = key // n, key % n
    # the two entries of a column of B are w_e a_i and -w_e a_j: weights w_e^2 log-uniform over 1.5 decades (the scaled entries
    # straddle the drop tolerance), node factors a_i of either sign (so are the entries of A) over half a decade
    a = np.exp(rng.uniform(np.log(0.3), 0.0, n)) * rng.choice([-1.0, 1.0], n)
    w = np.exp(rng.uniform(np.log(0.17), 0.0, len(lo)))
    w = np.where(weak[lo] | weak[hi], 0.03 * w, w)               # (a weak row must not pin its neighbours down: it would lift the smooth modes)
    bl, bh = w * a[lo], -w * a[hi]
    off = (bl * bh).astype(np.float32)                           # the upper triangle; mirrored below
    dsum = np.zeros(n)
    np.add.at(dsum, lo, bl * bl)
    np.add.at(dsum, hi, bh * bh)
    scale = max(float(dsum.mean()), 1e-2) if len(lo) else 1.0
    E = np.where(weak, 1e6 * np.maximum(dsum, scale * 1e-3), eps * np.maximum(dsum, scale * 1e-3) * rng.uniform(0.5, 2.0, n))
    diag = (dsum + E).astype(np.float32)
    dense = np.zeros((n, n), np.float32)
    dense[lo, hi] = off
    dense[hi, lo] = off
    dense[np.arange(n), np.arange(n)] = diag
    rowptr, cols, vals = csr_diag_last(dense, rng)
    return dict(rowptr=rowptr, cols=cols, vals=vals, diag=diag, row_seg=row_seg, nseg=nseg, n=n, dense=dense.astype(np.float64), weak=weak)


def csr_diag_last(dense, rng):
    """CSR of the non-zero pattern of a dense fp32 matrix: every row's off-diagonal columns in random order, its diagonal last."""
    n = dense.shape[0]
    rowptr = np.zeros(n + 1, np.int32)
    cols, vals = [], []
    for i in range(n):
        c = np.nonzero(dense[i])[0]
        c = rng.permutation(c[c != i])
        c = np.concatenate([c, [i]])
        cols.append(c)
        vals.append(dense[i, c])
        rowptr[i + 1] = rowptr[i] + len(c)
    return rowptr, np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(np.float32)


def interleaved(counts, seed):
    """row_seg with counts[c] rows of segment c in random (interleaved) order"""
    rs = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return np.random.default_rng(seed).permutation(rs) if len(counts) > 1 else rs


# the committed block set: name -> (segment sizes, seed, hubs).  n in {1, 15, 16, 17, 64, 65, 257, 1501}; one and three segments; a
# one-row segment; the large block holds every row length of HUB_DEGREES in its first segment and is no multiple of 16 (the last
# wavefront of the packed step is partly dead)
BLOCKS = {
    'n1': ((1,), 11, ()),
    'n15': ((15,), 12, ()),
    'n16': ((16,), 13, ()),
    'n17x3': ((9, 1, 7), 14, ()),
    'n64': ((64,), 15, ()),
    'n65x3': ((40, 1, 24), 16, ()),
    'n257': ((257,), 17, ()),
    'n1501x3': ((1000, 1, 500), 68, HUB_DEGREES),
}


@functools.lru_cache(maxsize=None)
def block(name):
    counts, seed, hubs = BLOCKS[name]
    b = make_block(interleaved(counts, seed), seed, hubs)
    b['name'] = name
    return b


def sub_block(blk, c):
    """segment c of a block as a block of its own (rows in their PCG order, columns renumbered, entry order kept) and its rows"""
    rows = np.nonzero(blk['row_seg'] == c)[0]
    local = np.full(blk['n'], -1, np.int64)
    local[rows] = np.arange(len(rows))
    lens = np.diff(blk['rowptr'])[rows]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    take = np.concatenate([np.arange(blk['rowptr'][j], blk['rowptr'][j + 1]) for j in rows])
    cols = local[blk['cols'][take]]
    assert (cols >= 0).all()
    return dict(rowptr=rowptr, cols=cols.astype(np.int32), vals=blk['vals'][take], diag=blk['diag'][rows], n=len(rows), nseg=1,
                row_seg=np.zeros(len(rows), np.int32), dense=blk['dense'][np.ix_(rows, rows)]), rows


# ---- the coefficient rule ---------------------------------------------------------------------------------------------------------
def interval_top(lam, gersh, scale):
    """upper end of every segment's interval in fp64 (the kernel's rule), NaN where the segment is degenerate"""
    lam = np.atleast_1d(np.asarray(lam, np.float32))
    with np.errstate(invalid='ignore', over='ignore'):
        lmax = np.float64(np.float32(scale)) * lam.astype(np.float64)
        if gersh is not None:
            g = np.atleast_1d(np.asarray(gersh, np.float32))
            cap = (g > 0) & (g.astype(np.float64) < lmax)
            lmax = np.where(cap, g.astype(np.float64), lmax)
        return np.where((lmax > 0.0) & (lmax < 1e30), lmax, np.nan)


def cheb_coeffs(lam, gersh, scale, ratio, steps):
    """k_cheb_coeffs: [nseg, STRIDE] fp32 table {1 / theta, a_0, b_0, a_1, b_1, ...} (entries past 2 * steps are left 0)"""
    top = interval_top(lam, gersh, scale)
    out = np.zeros((len(top), STRIDE), np.float32)
    for c, lmax in enumerate(top):
        if np.isnan(lmax):
            out[c, 0] = 1.0
            continue
        lmin = lmax / np.float64(np.float32(ratio))
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        sigma = theta / delta
        rho = 1.0 / sigma
        out[c, 0] = np.float32(1.0 / theta)
        for i in range(steps):
            rho_n = 1.0 / (2.0 * sigma - rho)
            out[c, 1 + 2 * i] = np.float32(rho_n * rho)
            out[c, 2 + 2 * i] = np.float32(2.0 * rho_n / delta)
            rho = rho_n
    return out


def cheb_T(k, x):
    """T_k(x) for any real x (three-term recurrence, fp64)"""
    x = np.asarray(x, np.float64)
    t0, t1 = np.ones_like(x), x
    if k == 0:
        return t0
    for _ in range(k - 1):
        t0, t1 = t1, 2.0 * x * t1 - t0
    return t1


def poly(l, lmax, ratio, steps):
    """p(l) of the interval [lmax / ratio, lmax]; p = 1 for a degenerate interval (lmax NaN)"""
    l = np.asarray(l, np.float64)
    if np.isnan(lmax):
        return np.ones_like(l)
    lmin = lmax / np.float64(np.float32(ratio))
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    return (1.0 - cheb_T(steps, (theta - l) / delta) / cheb_T(steps, theta / delta)) / l


# ---- the operator -----------------------------------------------------------------------------------------------------------------
def eig_segments(S, row_seg):
    """[(rows, eigenvalues, eigenvectors)] of every segment's block of the symmetric matrix S"""
    out = []
    for c in range(int(np.max(row_seg)) + 1 if len(row_seg) else 0):
        rows = np.nonzero(row_seg == c)[0]
        w, U = np.linalg.eigh(S[np.ix_(rows, rows)])
        out.append((rows, w, U))
    return out


def closed_form_scaled(eigs, dis, r, top, ratio, steps):
    """z = dis U p(lam) U^T dis r per segment, fp64; eigs = eig_segments(S, row_seg), top = interval_top(...)"""
    r = np.asarray(r, np.float64)
    z = np.zeros_like(r)
    for (rows, w, U), lmax in zip(eigs, top):
        z[rows] = dis[rows] * (U @ (poly(w, lmax, ratio, steps) * (U.T @ (dis[rows] * r[rows]))))
    return z


def apply_closed_form(A, D, r, row_seg, top, ratio, steps):
    """The eigen-decomposition formula of the module docstring for the dense matrix A with diagonal D."""
    dis = 1.0 / np.sqrt(np.asarray(D, np.float64))
    S = np.asarray(A, np.float64) * dis[:, None] * dis[None, :]
    return closed_form_scaled(eig_segments(0.5 * (S + S.T), row_seg), dis, r, top, ratio, steps)


def _rowsum(rowptr, prod):
    """sum of prod over every row's entries in storage order (rows may be empty)"""
    out = np.zeros(len(rowptr) - 1, prod.dtype)
    lens = np.diff(rowptr)
    if len(prod):
        nz = lens > 0
        out[nz] = np.add.reduceat(prod, rowptr[:-1][nz])
    return out


def apply_recurrence(rowptr, cols, vals, D, r, coef, row_seg, steps, dtype, dis=None):
    """The recurrence as the kernel comment states it, every operation rounded to `dtype`.
    dis None: plain block (vals hold the diagonal).  dis given: the scaled variables of the packed block -- rowptr / cols / vals are
    then the off-diagonal entries of S_h over the PCG-order unknowns, and the unit diagonal is added as the kernel adds it."""
    f = dtype
    vals, r, coef = np.asarray(vals).astype(f), np.asarray(r).astype(f), np.asarray(coef, np.float32).astype(f)
    seg = np.zeros(len(r), np.int64) if row_seg is None else np.asarray(row_seg, np.int64)
    c0 = coef[seg, 0]
    if dis is None:
        D = np.asarray(D).astype(f)
        res, d, y = r.copy(), (r / D * c0).astype(f), np.zeros_like(r)
        for i in range(steps):
            t = _rowsum(rowptr, vals * d[cols])
            y = y + d
            res = res - t
            d = (coef[seg, 1 + 2 * i] * d + coef[seg, 2 + 2 * i] * res / D).astype(f)
        return y
    dis = np.asarray(dis).astype(f)
    res = (r * dis).astype(f)
    d, y = (res * c0).astype(f), np.zeros_like(r)
    for i in range(steps):
        t = _rowsum(rowptr, vals * d[cols]) + d
        y = y + d
        res = res - t
        d = (coef[seg, 1 + 2 * i] * d + coef[seg, 2 + 2 * i] * res).astype(f)
    return (y * dis).astype(f)


# ---- the packer -------------------------------------------------------------------------------------------------------------------
def pack_ref(rowptr, cols, vals, diag, row_seg, drop):
    """format 1 of nksr_coarse_precond_t from the plain block, built as fields/coarse_precond.py:_pack_block builds it.
    -> dict: packed (uint32 words), packed_rowptr, lens, dis (fp32, new order), old_of_new, new_of_old, seg_base, row_seg_new,
    S_h (dense fp64, PCG order, unit diagonal: the matrix the words denote), s32 (the fp32 products before the rounding to half, per
    off-diagonal entry of the plain block in storage order), csr (rowptr, cols, vals of S_h's kept off-diagonal entries, PCG order)."""
    rowptr, cols = np.asarray(rowptr, np.int64), np.asarray(cols, np.int64)
    vals, diag = np.asarray(vals, np.float32), np.asarray(diag, np.float32)
    n = len(diag)
    row_seg = np.zeros(n, np.int32) if row_seg is None else np.asarray(row_seg, np.int32)
    nseg = int(row_seg.max()) + 1
    old_of_new = np.argsort(row_seg.astype(np.int64) * n + np.arange(n), kind='stable')
    new_of_old = np.empty(n, np.int64)
    new_of_old[old_of_new] = np.arange(n)
    counts = np.bincount(row_seg, minlength=nseg)
    seg_base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    row_seg_new = row_seg[old_of_new]
    dis_old = (np.float32(1.0) / np.sqrt(diag)).astype(np.float32)
    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    offd = np.ones(len(cols), bool)
    offd[rowptr[1:] - 1] = False                                   # the diagonal closes every row
    assert (cols[~offd] == np.arange(n)).all(), 'every row must hold its diagonal as its last entry'
    s32 = (vals * (dis_old[row_of] * dis_old[cols]).astype(np.float32)).astype(np.float32)
    sh = s32.astype(np.float16)
    keep = offd & (np.abs(sh.astype(np.float32)) >= np.float32(drop))
    word = (sh.view(np.uint16).astype(np.uint32) << np.uint32(16)) | (new_of_old[cols] - seg_base[row_seg[row_of]]).astype(np.uint32)
    assert (new_of_old[cols] - seg_base[row_seg[row_of]] < 65536).all() and (new_of_old[cols] >= seg_base[row_seg[row_of]]).all()
    lens_old = np.bincount(row_of[keep], minlength=n)
    lens = lens_old[old_of_new].astype(np.int32)
    prow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    # entries in new row order, kept entries in their storage order
    order = np.argsort(new_of_old[row_of[keep]], kind='stable')
    packed = word[keep][order].astype(np.uint32)
    S_h = np.zeros((n, n))
    S_h[row_of[keep], cols[keep]] = sh[keep].astype(np.float64)
    S_h[np.arange(n), np.arange(n)] = 1.0
    csr = (np.concatenate([[0], np.cumsum(lens_old)]).astype(np.int64), cols[keep], sh[keep].astype(np.float32))
    return dict(packed=packed, packed_rowptr=prow, lens=lens, dis=dis_old[old_of_new], dis_old=dis_old, old_of_new=old_of_new.astype(np.int32),
                new_of_old=new_of_old.astype(np.int32), seg_base=seg_base, row_seg_new=row_seg_new.astype(np.int32), S_h=S_h,
                s32=s32[offd], csr=csr, nseg=nseg, n=n)


def half_ulp_at(x):
    """spacing of the half-precision numbers around x (normal range)"""
    return float(np.spacing(np.float16(x)))


def drop_margin(s32, drop):
    """smallest distance of an fp32 scaled entry from the drop tolerance, in half-precision ulps at the tolerance: above 1, the value
    rounds to a half that lies strictly on its own side of `drop`, and one fp32 ulp more or less would not change the decision"""
    if drop <= 0 or len(s32) == 0:
        return np.inf
    return float(np.min(np.abs(np.abs(s32.astype(np.float64)) - float(np.float32(drop)))) / half_ulp_at(drop))


# ---- eigenvalue bounds ------------------------------------------------------------------------------------------------------------
def power_ref(apply, n, row_seg, iters, dtype=np.float64):
    """`iters` (>= 2) steps v <- apply(v) from all ones; ||v_k|| / ||v_{k-1}|| per segment (norms in fp64, as the kernel's), 0 for a
    segment without rows"""
    iters = max(int(iters), 2)
    v = [np.ones(n, dtype)]
    for _ in range(iters):
        v.append(apply(v[-1]).astype(dtype))
    a, b = v[-2].astype(np.float64), v[-1].astype(np.float64)
    nseg = int(np.max(row_seg)) + 1 if len(row_seg) else 1
    out = np.zeros(nseg)
    for c in range(nseg):
        m = row_seg == c
        sa, sb = float((a[m] ** 2).sum()), float((b[m] ** 2).sum())
        out[c] = np.sqrt(sb / sa) if sa > 0 else 0.0
    return out


def power_plain(blk, iters, dtype=np.float64, row_seg=None):
    """v <- D^-1 A v (format 0)"""
    rowptr, cols = blk['rowptr'], blk['cols']
    vals, D = blk['vals'].astype(dtype), blk['diag'].astype(dtype)
    rs = np.zeros(blk['n'], np.int64) if row_seg is None else row_seg
    return power_ref(lambda v: _rowsum(rowptr, vals * v[cols]) / D, blk['n'], rs, iters, dtype)


def power_packed(pk, iters, dtype=np.float64):
    """v <- S_h v (packed; segment-wise, so the order of the unknowns does not matter)"""
    rowptr, cols, vals = pk['csr']
    vals = vals.astype(dtype)
    rs = np.empty(pk['n'], np.int64)
    rs[pk['old_of_new']] = pk['row_seg_new']
    return power_ref(lambda v: _rowsum(rowptr, vals * v[cols]) + v, pk['n'], rs, iters, dtype)


def gersh_ref(blk=None, pk=None, row_seg=None, dtype=np.float64):
    """Gershgorin bound per segment: max_i sum_j |a_ij| / d_i (plain, the diagonal included) or 1 + sum_j |S_h ij| (packed)"""
    if pk is not None:
        rowptr, cols, vals = pk['csr']
        rows = (np.asarray(1, dtype) + _rowsum(rowptr, np.abs(vals).astype(dtype)))
        rs = np.empty(pk['n'], np.int64)
        rs[pk['old_of_new']] = pk['row_seg_new']
    else:
        rows = _rowsum(blk['rowptr'], np.abs(blk['vals']).astype(dtype)) / blk['diag'].astype(dtype)
        rs = np.zeros(blk['n'], np.int64) if row_seg is None else np.asarray(row_seg, np.int64)
    return np.array([rows[rs == c].max() if (rs == c).any() else 0.0 for c in range(int(rs.max()) + 1)], np.float64)


def lambda_true(S, row_seg):
    """largest eigenvalue of every segment's block of the symmetric S"""
    return np.array([w[-1] for _, w, _ in eig_segments(S, row_seg)])


def scaled_dense(blk):
    """S = D^-1/2 A D^-1/2 of a plain block in fp64, and D^-1/2"""
    dis = 1.0 / np.sqrt(blk['diag'].astype(np.float64))
    S = blk['dense'] * dis[:, None] * dis[None, :]
    return 0.5 * (S + S.T), dis


def rel_err(z, ref, row_seg):
    """max-abs error over max |ref|, the worst segment"""
    z, ref = np.asarray(z, np.float64), np.asarray(ref, np.float64)
    rs = np.zeros(len(ref), np.int64) if row_seg is None else np.asarray(row_seg)
    worst = 0.0
    for c in range(int(rs.max()) + 1):
        m = rs == c
        if m.any():
            worst = max(worst, float(np.abs(z[m] - ref[m]).max() / max(np.abs(ref[m]).max(), 1e-300)))
    return worst


# ---- what the CPU and the GPU tests share ----------------------------------------------------------------------------------------
RATIO, SCALE, STEPS = 40.0, 1.1, (1, 2, 8, 10, 16)
BOUND_BLOCKS = ('n257', 'n1501x3', 'ranges')      # the blocks the eigenvalue-bound tests run on (test_coarse_precond_cpu.py says why)


@functools.lru_cache(maxsize=None)
def ranges_block():
    """A block whose segments are index ranges, as nksr_segments_t describes them: two "levels" of coarse rows, each holding one range
    per segment, behind `first` finer unknowns.  Segment 3 has rows on the fine level only: both its coarse ranges are empty.
    -> (block, first, lo [4 * 3], hi [4 * 3]) with lo / hi in unknown indices (range k of segment c at c * 3 + k)."""
    first = 37
    sizes = ((60, 41, 50, 0), (30, 1, 22, 0))                         # rows of segments 0..3 on the two coarse levels
    fine = (10, 9, 8, 10)                                             # and on the fine level: [0, first)
    lo, hi = np.zeros((4, 3), np.int32), np.zeros((4, 3), np.int32)
    at = 0
    for c in range(4):
        lo[c, 0], hi[c, 0] = at, at + fine[c]
        at += fine[c]
    assert at == first
    rs = []
    for k, lv in enumerate(sizes):
        for c in range(4):
            lo[c, 1 + k], hi[c, 1 + k] = at, at + lv[c]
            at += lv[c]
            rs += [c] * lv[c]
    b = make_block(np.asarray(rs, np.int32), 21)
    b['name'] = 'ranges'
    return b, first, lo.reshape(-1), hi.reshape(-1)

DROP = 0.005              # fields/coarse_precond.py: PC_DROP_TOL (the GPU test asserts that it still is)


@functools.lru_cache(maxsize=None)
def prepared(name, fmt, drop=0.0):
    """A block of the set with everything the references need, computed once: the scaled matrix of the format (S, or S_h of
    pack_ref), D^-1/2 as the kernels hold it, the eigenpairs of every segment and lam [nseg] fp32 = every segment's largest eigenvalue
    (what the tests pass as `lambda`: the interval is then the test's own, and differs from segment to segment)."""
    blk = ranges_block()[0] if name == 'ranges' else block(name)
    pk = None
    if fmt == 0:
        S, dis = scaled_dense(blk)
    else:
        pk = pack_ref(blk['rowptr'], blk['cols'], blk['vals'], blk['diag'], blk['row_seg'], drop)
        S, dis = pk['S_h'], pk['dis_old'].astype(np.float64)
    eigs = eig_segments(S, blk['row_seg'])
    lam = np.array([w[-1] for _, w, _ in eigs], np.float32)
    return dict(blk=blk, pk=pk, S=S, dis=dis, eigs=eigs, lam=lam, fmt=fmt, drop=drop)


def rhs(n, seed=0):
    return np.random.default_rng(1000 + seed).standard_normal(n).astype(np.float32)


def reference(prep, r, steps, lam=None, gersh=None, scale=SCALE, ratio=RATIO, dtype=None):
    """dtype None: the closed form (fp64).  Otherwise the recurrence of the block's format in that precision, with the fp32 table."""
    blk, pk = prep['blk'], prep['pk']
    lam = prep['lam'] if lam is None else lam
    if dtype is None:
        return closed_form_scaled(prep['eigs'], prep['dis'], r, interval_top(lam, gersh, scale), ratio, steps)
    coef = cheb_coeffs(lam, gersh, scale, ratio, steps)
    if pk is None:
        return apply_recurrence(blk['rowptr'], blk['cols'], blk['vals'], blk['diag'], r, coef, blk['row_seg'], steps, dtype)
    rp, cols, vals = pk['csr']
    return apply_recurrence(rp, cols, vals, None, r, coef, blk['row_seg'], steps, dtype, dis=pk['dis_old'])


def rounding_floor(prep, r, steps, **kw):
    """(closed form, error of the fp32 recurrence against it: max-abs over max |z_ref|, worst segment -- never below the unit roundoff
    of fp32, which no fp32 evaluation is expected to beat and which a one-row segment can reach by luck)"""
    zref = reference(prep, r, steps, **kw)
    z32 = reference(prep, r, steps, dtype=np.float32, **kw)
    return zref, max(rel_err(z32, zref, prep['blk']['row_seg']), U32)
