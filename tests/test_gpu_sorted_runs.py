"""ops.sorted_runs (csrc/prims.hip: k_run_counts, k_run_table) alone, against a numpy restatement: the run table of sorted 64-bit keys
that the edge table, the simplifier's clusters and the voxel grouping share.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
MID = 1 << 40
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1031]      # round the wavefront (64) and the block (256); several blocks


def runs_ref(k, none_from):
    """(n_runs, start [R + 1], run keys [R], run_of [n]) of sorted uint64 keys."""
    inside = k < np.uint64(none_from)
    head = inside & np.concatenate([[True], k[1:] != k[:-1]])[:len(k)]
    run_of = np.where(inside, np.cumsum(head) - 1, -1)
    start = np.append(np.flatnonzero(head), inside.sum())              # (sorted: the keys >= none_from are a tail)
    return int(head.sum()), start, k[head], run_of


def from_heads(head, step=3):
    return (np.cumsum(head) * step).astype(np.uint64)


def random_runs(n, rng):
    """runs of random length 1 .. 5"""
    head = np.zeros(n, bool)
    i = 0
    while i < n:
        head[i] = True
        i += int(rng.integers(1, 6))
    return from_heads(head)


def cases(n):
    """(name, sorted uint64 keys [n], none_from)"""
    rng = np.random.default_rng(n)
    shapes = {'equal': np.full(n, 7, np.uint64), 'distinct': np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1),
              'random runs': random_runs(n, rng)}
    spanning = np.full(n, 5, np.uint64)                                 # one run across every block edge, a short one at either end
    if n >= 3:
        spanning[0], spanning[-1] = 1, 9
    shapes['spanning'] = spanning
    head = np.zeros(n, bool)                                            # runs of length 1 at the last lane of a wavefront / block and the first of the next
    for p in (0, 63, 64, 65, 255, 256, 257):
        if p < n:
            head[p] = True
    shapes['singles at 63, 64, 255, 256'] = from_heads(head)
    high = random_runs(n, rng)
    high[n // 2:] |= np.uint64(1 << 63)                                 # unsigned order: these sort last, as int64 they are negative
    shapes['bit 63'] = high
    for name, k in shapes.items():
        yield name, k, U64_MAX
        yield name + ', none_from = the middle key', k, int(k[n // 2]) if n else MID
        yield name + ', none_from below every key', k, 0
    for t in sorted({0, 255, 256, 257, n}):                             # a tail that belongs to no run, from position t on (t = 0: nothing but the tail)
        if t > n:
            continue
        body = random_runs(t, rng)
        yield 'all-ones tail from %d' % t, np.concatenate([body, np.full(n - t, U64_MAX, np.uint64)]), U64_MAX
        tail = np.uint64(MID) + (np.arange(n - t, dtype=np.uint64) // np.uint64(2))       # (several keys >= none_from, repeated ones too)
        yield 'tail from %d' % t, np.concatenate([body, tail]), MID


def device_keys(k):
    return torch.from_numpy(k.view(np.int64).copy()).to('cuda:0')


@pytest.mark.parametrize('n', SIZES)
def test_sorted_runs_matches_the_restatement(n):
    from nksr_amd import ops
    count = 0
    for name, k, none_from in cases(n):
        assert len(k) == n and bool((k[1:] >= k[:-1]).all()), name
        nr, start, keys, run_of = runs_ref(k, none_from)
        want_start = torch.from_numpy(start.astype(np.int32))
        want_keys = torch.from_numpy(keys.view(np.int64).copy())
        want_of = torch.from_numpy(run_of.astype(np.int32))
        ks = device_keys(k)
        for with_keys in (False, True):
            for with_of in (False, True):
                every = none_from == U64_MAX and with_keys                 # (the default and the value written out are the same thing)
                got = ops.sorted_runs(ks, none_from=None if every else none_from, keys=with_keys, run_of=with_of)
                what = (name, n, with_keys, with_of)
                assert got[0] == nr, what
                assert got[1].dtype == torch.int32 and torch.equal(got[1].cpu(), want_start), what
                assert (got[2] is None) == (not with_keys) and (got[3] is None) == (not with_of), what
                if with_keys:
                    assert got[2].dtype == torch.int64 and torch.equal(got[2].cpu(), want_keys), what
                if with_of:
                    assert got[3].dtype == torch.int32 and torch.equal(got[3].cpu(), want_of), what
                count += 1
    assert count >= 4 * (18 + 2 * (1 if n == 0 else 2))


def test_the_two_entry_points_and_the_block_count_layout():
    """block_counts is [blocks + 1]: heads per block of 256 positions, then a 0 that the entry point writes; its exclusive sum ends with
    n_runs, which nksr_run_table_u64 takes from the caller."""
    from nksr_amd import ops
    from nksr_amd._lib import call, lib, ptr, stream
    dev = torch.device('cuda:0')
    n = 1031
    k = np.concatenate([random_runs(n - 100, np.random.default_rng(5)), np.full(100, MID + 1, np.uint64)])
    nr, start, keys, run_of = runs_ref(k, MID)
    nb = int(lib.nksr_run_blocks(n))
    assert nb == 5
    ks = device_keys(k)
    counts = torch.full((nb + 1,), -7, dtype=torch.int64, device=dev)
    call('nksr_run_counts_u64', ptr(ks), n, MID, ptr(counts), stream())
    head = run_of != np.concatenate([[-1], run_of[:-1]])
    head &= run_of >= 0
    want_counts = [int(head[b * 256:(b + 1) * 256].sum()) for b in range(nb)] + [0]
    assert counts.tolist() == want_counts
    offsets = ops.exclusive_sum_i64(counts)
    assert int(offsets[nb].item()) == nr
    got_start = torch.full((nr + 1,), -7, dtype=torch.int32, device=dev)
    got_keys = torch.full((nr,), -7, dtype=torch.int64, device=dev)
    got_of = torch.full((n,), -7, dtype=torch.int32, device=dev)
    call('nksr_run_table_u64', ptr(ks), n, MID, ptr(offsets), nr, ptr(got_start), ptr(got_keys), ptr(got_of), stream())
    assert got_start.tolist() == start.tolist() and got_keys.tolist() == keys.astype(np.int64).tolist() and got_of.tolist() == run_of.tolist()
    # n = 0: the closing entries alone, keys and offsets may be NULL
    call('nksr_run_counts_u64', None, 0, U64_MAX, ptr(counts), stream())
    call('nksr_run_table_u64', None, 0, U64_MAX, None, 0, ptr(got_start), None, None, stream())
    assert int(counts[0].item()) == 0 and int(got_start[0].item()) == 0
