"""nksr_amd/fields/row_layout.py (the row layout of the matrix-free operator: pure integer torch) against a numpy statement of the
same layout written here: a stable argsort of the concatenated keys (set 0 first on equal keys), a cumulative sum of the rows
per site, every segment started on the next multiple of 256.  No GPU."""
import types

import numpy as np
import pytest
import torch

from nksr_amd.fields.row_layout import first_rows_from_ranks, pad_segments


def _segments(key_lo):
    """What pad_segments needs of a Segments object: key_lo, nseg, of_keys."""
    klo = torch.from_numpy(np.asarray(key_lo, np.int64))
    return types.SimpleNamespace(key_lo=klo, nseg=len(key_lo), of_keys=lambda k: torch.bucketize(k, klo, right=True) - 1)


def _numpy_layout(keys, rps, key_lo=None):
    """(first rows per set, rows_total, pad_rows, item_seg, segment starts) by sorting."""
    allk = np.concatenate(keys)
    rows_site = np.concatenate([np.full(len(k), c, np.int64) for k, c in zip(keys, rps)])
    order = np.argsort(allk, kind='stable')                      # the concatenation puts set 0 first: stable keeps it first on ties
    first_sorted = np.cumsum(rows_site[order]) - rows_site[order]
    total = int(rows_site.sum())
    if key_lo is None:
        first = np.empty(len(allk), np.int64)
        first[order] = first_sorted
        return np.split(first, [len(keys[0])]) if len(keys) == 2 else [first], total, None, None, None
    ks = allk[order]
    seg_sorted = np.searchsorted(np.asarray(key_lo), ks, side='right') - 1
    first_sorted = first_sorted.copy()
    cursor, starts, pad_rows = 0, [], []
    for s in range(len(key_lo)):
        lo = np.searchsorted(ks, key_lo[s], side='left')
        hi = np.searchsorted(ks, key_lo[s + 1], side='left') if s + 1 < len(key_lo) else len(ks)
        nrows = int(rows_site[order][lo:hi].sum())
        starts.append(cursor)
        unpadded = int(first_sorted[lo]) if hi > lo else 0
        first_sorted[lo:hi] += cursor - unpadded
        end = cursor + nrows
        cursor = -(-end // 256) * 256
        pad_rows += list(range(end, cursor))
    first = np.empty(len(allk), np.int64)
    first[order] = first_sorted
    assert (seg_sorted >= 0).all()
    item_seg = np.searchsorted(np.asarray(starts), 32 * np.arange(cursor // 32 + 2), side='right') - 1
    first = np.split(first, [len(keys[0])]) if len(keys) == 2 else [first]
    return first, cursor, np.asarray(pad_rows, np.int64), np.clip(item_seg, 0, len(key_lo) - 1), starts


def _torch_layout(keys, rps, key_lo=None):
    tk = [torch.from_numpy(k) for k in keys]
    if len(keys) == 2:
        ra = torch.from_numpy(np.searchsorted(keys[1], keys[0], side='left').astype(np.int32))
        rb = torch.from_numpy(np.searchsorted(keys[0], keys[1], side='right').astype(np.int32))
        first = list(first_rows_from_ranks(len(keys[0]), len(keys[1]), ra, rb, rps[0], rps[1]))
    else:
        first = [torch.arange(len(keys[0]), dtype=torch.int32) * rps[0]]
    if key_lo is None:
        return first, sum(len(k) * c for k, c in zip(keys, rps)), None, None
    return pad_segments(first, tk, list(rps), _segments(key_lo))


def _keys(rs, n, hi=2000):
    return np.sort(rs.randint(0, hi, n)).astype(np.int64)       # (n > hi / 2: runs of equal keys inside a set and across the sets)


def _cases():
    rs = np.random.RandomState(11)
    cases = []
    for rps in ((1, 3), (1, 4)):
        for na, nb in ((0, 0), (1, 0), (0, 1), (1, 1), (400, 397), (403, 1), (0, 400)):
            for key_lo in (None, [0], [0, 700], [0, 500, 1000, 1500, 1900], [0, 0, 900], [0, 900, 900, 1500], [0, 900, 2000]):
                cases.append(([_keys(rs, na), _keys(rs, nb)], rps, key_lo))         # ([0, 0, ..]: empty first, [.., 900, 900, ..]: empty middle,
                cases.append(([_keys(rs, na)], rps[:1], key_lo))                    # [.., 2000]: empty last segment -- keys are < 2000)
                cases.append(([_keys(rs, nb)], rps[1:], key_lo))
    # a segment whose row count is a multiple of 256 already: 64 position + 64 normal sites (1 + 3 rows) = 256 rows, then a second segment
    a = np.concatenate([np.arange(64), 100 + np.arange(10)]).astype(np.int64)
    b = np.concatenate([np.arange(64), 100 + np.arange(7)]).astype(np.int64)
    cases.append(([a, b], (1, 3), [0, 100]))
    cases.append(([np.repeat(np.arange(8), 8).astype(np.int64)], (4,), [0, 8]))      # 64 sites x 4 rows = 256, one set, empty last segment
    return cases


def test_first_rows_and_segment_padding_equal_the_sorted_statement():
    nseg_seen, no_pad_seen = set(), False
    for keys, rps, key_lo in _cases():
        first, total, pad_rows, item_seg = _torch_layout(keys, rps, key_lo)
        rfirst, rtotal, rpad, ritem, starts = _numpy_layout(keys, rps, key_lo)
        assert total == rtotal, (rps, key_lo)
        for f, r in zip(first, rfirst):
            assert f.dtype == torch.int32 and np.array_equal(f.numpy().astype(np.int64), r), (rps, key_lo)
        if key_lo is None:
            assert pad_rows is None and item_seg is None
            continue
        nseg_seen.add(len(key_lo))
        assert np.array_equal(pad_rows.numpy(), rpad) and item_seg.dtype == torch.int32 and np.array_equal(item_seg.numpy(), ritem)
        # properties, stated without the reference: segment starts are multiples of 256 ...
        klo = np.asarray(key_lo)
        owned = np.zeros(total, bool)
        for k, f, c in zip(keys, first, rps):
            seg = np.searchsorted(klo, k, side='right') - 1
            rows = f.numpy().astype(np.int64)[:, None] + np.arange(c)[None]
            for s in np.unique(seg):
                assert rows[seg == s].min() >= starts[s] and starts[s] % 256 == 0
                if s + 1 < len(klo):
                    assert rows[seg == s].max() < starts[s + 1]
            assert not owned[rows.reshape(-1)].any()            # (no row has two owners)
            owned[rows.reshape(-1)] = True
        # ... the pad rows are exactly the rows no site owns ...
        assert np.array_equal(np.nonzero(~owned)[0], pad_rows.numpy())
        # ... and item i is the segment of rows 32 i .. 32 i + 31 (segments start on multiples of 256: an item never straddles two)
        row_seg = np.searchsorted(np.asarray(starts), np.arange(total), side='right') - 1
        assert item_seg.numel() == total // 32 + 2
        for i in range(total // 32):
            assert (row_seg[32 * i:32 * i + 32] == item_seg[i].item()).all()
        no_pad_seen |= bool(len(key_lo) > 1 and starts[1] == 256 and (np.asarray(rpad) >= 256).all())
    assert nseg_seen == {1, 2, 3, 4, 5} and no_pad_seen


@pytest.mark.parametrize('rps', [(1, 3), (1, 4)])
def test_ranks_merge_equal_keys_with_set_0_first(rps):
    ka, kb = np.array([5, 5, 7], np.int64), np.array([5, 5, 6, 7], np.int64)
    first, total, _, _ = _torch_layout([ka, kb], rps)
    c = rps[1]
    assert total == 3 + 4 * c
    assert first[0].tolist() == [0, 1, 2 + 3 * c] and first[1].tolist() == [2, 2 + c, 2 + 2 * c, 3 + 3 * c]
