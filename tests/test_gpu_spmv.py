"""The streaming CSR SpMV (csrc/spmv.hip: k_spmv_plan, k_spmv, k_spmv_fixup) alone, through solver.spmv, on hand-built CSRs in both
physical layouts (tests/spmv_layout.py; format 1 is packed by nksr_pack_cols21).  The kernel cuts the entry stream into chunks of
C = 4096 (format 0) / 4608 (format 1) entries regardless of rows, so what can go wrong sits where rows meet chunk boundaries; every
structure below is built from C, so that its edge falls at the same place in both formats.

The kernel's contract: every row holds at least one entry (its diagonal).  Rows of length 0 are outside it and are not tested.

Exact cases: values are integers in [-4, 4] and x integers in [-8, 8], both as fp32.  The longest row has 2.5 x 4608 entries with
|product| <= 32, so every partial sum stays below 2^24 in magnitude and the fp32 result is exact in any order of summation: it must
equal the int64 reference.  Rounded cases: the same structures with normal values and x against the fp64 product, within the
project's SpMV bound |y - y64| <= 1e-5 (|A| |x|) per row (tests/test_gpu_parity.py)."""
import functools

import numpy as np
import pytest
import torch

import spmv_layout

pytestmark = pytest.mark.gpu


def _short(rng, total):
    """row lengths 1..6 that sum to exactly `total`"""
    out, left = [], total
    while left > 0:
        n = min(int(rng.integers(1, 7)), left)
        out.append(n)
        left -= n
    return out


def _structure(case, C, rng):
    """row lengths of one case (every row >= 1)"""
    if case == 'short_rows':        # ~ one chunk in which far more than 256 rows start: the branch that reloads row pointers (j >= 64)
        return [int(n) for n in rng.integers(1, 7, 1200)]
    if case == 'long_row':          # head in chunk 0 from entry C / 2, then all of chunks 1 and 2: one carry run over two chunks
        return _short(rng, C // 2) + [5 * C // 2] + _short(rng, 300)
    if case == 'boundary_rows':     # a row whose last entry is C - 1, the next one starting at entry C; the same at 2 C after a longer row
        return _short(rng, C) + [7] + _short(rng, C - 7 - 40) + [40] + [3] + _short(rng, 200)
    if case == 'two_long_rows':     # 1.5 C and 1.25 C back to back from 0.75 C: neighbouring chunks carry for different rows;
        #                             then one row that is exactly chunk 4
        return _short(rng, 3 * C // 4) + [3 * C // 2, 5 * C // 4] + _short(rng, C // 2) + [C] + _short(rng, 100)
    if case == 'one_entry':
        return [1]
    if case == 'nnz_multiple':      # nnz = 2 C exactly: no padding at all
        return _short(rng, 2 * C)
    if case == 'nnz_plus_one':      # nnz = C + 1: the last chunk holds a single entry
        return _short(rng, C + 1)
    raise ValueError(case)


CASES = ['short_rows', 'long_row', 'boundary_rows', 'two_long_rows', 'one_entry', 'nnz_multiple', 'nnz_plus_one']
PARAMS = [(f, c) for f in (0, 1) for c in CASES]
IDS = ['fmt%d-%s' % p for p in PARAMS]


@functools.lru_cache(maxsize=None)
def _matrix(fmt, case):
    """(rowptr, cols: numpy; device rowptr) of one case: seeded, columns uniform in [0, M)"""
    C = spmv_layout.CHUNK[fmt]
    rng = np.random.default_rng(1000 + CASES.index(case))
    lens = np.asarray(_structure(case, C, rng), np.int64)
    assert lens.min() >= 1
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    M, nnz = len(lens), int(rowptr[-1])
    if case == 'long_row':
        assert rowptr[np.argmax(lens)] == C // 2 and rowptr[np.argmax(lens) + 1] == 3 * C
    if case == 'boundary_rows':
        assert C in rowptr and 2 * C in rowptr
    if case == 'two_long_rows':
        i = int(np.argmax(lens))
        assert rowptr[i] == 3 * C // 4 and lens[i + 1] == 5 * C // 4 and 4 * C in rowptr and 5 * C in rowptr
    if case == 'nnz_multiple':
        assert nnz == 2 * C
    if case == 'nnz_plus_one':
        assert nnz == C + 1
    cols = rng.integers(0, M, nnz).astype(np.int64)
    return rowptr, cols, torch.from_numpy(rowptr.astype(np.int32)).cuda()


def _product(fmt, case, vals, x):
    """solver.spmv of the case's structure with these values (numpy fp32) in the physical layout of `fmt`"""
    from nksr_amd import _lib, solver
    rowptr, cols, rowptr_d = _matrix(fmt, case)
    if fmt == 0:
        c, v = spmv_layout.encode0(cols, vals)
        cols_d = torch.from_numpy(c).cuda()
    else:
        c, v = spmv_layout.encode1(cols, vals)
        c32 = torch.from_numpy(c.astype(np.int32)).cuda()
        cols_d = torch.empty(len(c) // 3, dtype=torch.int64, device='cuda')
        _lib.call('nksr_pack_cols21', _lib.ptr(c32), len(c), _lib.ptr(cols_d), _lib.stream())
    assert len(c) % spmv_layout.CHUNK[fmt] == 0 and solver.col_format(cols_d) == fmt
    return solver.spmv(rowptr_d, cols_d, torch.from_numpy(v).cuda(), torch.from_numpy(x).cuda()).cpu().numpy()


def _values(fmt, case, integer):
    rowptr, cols, _ = _matrix(fmt, case)
    rng = np.random.default_rng(7 + CASES.index(case))
    M, nnz = len(rowptr) - 1, len(cols)
    if integer:
        return rng.integers(-4, 5, nnz).astype(np.float32), rng.integers(-8, 9, M).astype(np.float32)
    return rng.standard_normal(nnz).astype(np.float32), rng.standard_normal(M).astype(np.float32)


@pytest.mark.parametrize('fmt,case', PARAMS, ids=IDS)
def test_spmv_exact_on_small_integers(fmt, case):
    rowptr, cols, _ = _matrix(fmt, case)
    vals, x = _values(fmt, case, True)
    y = _product(fmt, case, vals, x)
    ref = np.add.reduceat(vals.astype(np.int64) * x.astype(np.int64)[cols], rowptr[:-1])
    assert np.abs(np.add.reduceat(np.abs(vals.astype(np.int64) * x.astype(np.int64)[cols]), rowptr[:-1])).max() < 2 ** 24
    bad = np.flatnonzero(y.astype(np.int64) != ref)
    assert np.array_equal(y, ref.astype(np.float32)) and bad.size == 0, (bad[:8], y[bad[:8]], ref[bad[:8]], rowptr[bad[:8]])


@pytest.mark.parametrize('fmt,case', PARAMS, ids=IDS)
def test_spmv_rounded_within_the_project_bound(fmt, case):
    rowptr, cols, _ = _matrix(fmt, case)
    vals, x = _values(fmt, case, False)
    y = _product(fmt, case, vals, x)
    prod = vals.astype(np.float64) * x.astype(np.float64)[cols]
    y64 = np.add.reduceat(prod, rowptr[:-1])
    bound = 1e-5 * np.add.reduceat(np.abs(prod), rowptr[:-1])
    err = np.abs(y - y64)
    print('spmv[fmt%d-%s]: max |y - y64| / (|A||x|) = %.3g (bound 1e-5)' % (fmt, case, (err / (bound / 1e-5)).max()))
    assert (err <= bound).all(), np.flatnonzero(err > bound)[:8]


@pytest.mark.parametrize('fmt,case', PARAMS, ids=IDS)
def test_spmv_is_deterministic(fmt, case):
    vals, x = _values(fmt, case, False)
    a, b = _product(fmt, case, vals, x), _product(fmt, case, vals, x)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
