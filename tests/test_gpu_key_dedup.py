"""nksr_footprint_keys_dedup (csrc/hierarchy.hip, k_footprint_dedup) by itself.

A workgroup takes a contiguous range of several batches of elements through ONE LDS hash set and emits the set -- one ticket on
the stream's counter -- only when the next batch might not fit (more than 1024 occupied slots; a batch holds at most 2048 keys) and
at the end of its range.  The contract: keys_out[0 .. count) is contiguous, holds the SET of keys of the plain stream (in any
order, a key possibly more than once), count <= the plain stream's length = the capacity of keys_out.

The mode-3 streams (the keys themselves) aim at the flush logic: streams around one batch, all-distinct streams (every batch
flushes), one key repeated (the set never flushes before the end), a cycle that fills the set across batches, and streams around
a workgroup's whole range (small streams: 4 batches of 2048 keys).  Modes 0, 1, 2 and the point source are compared with the
plain streams of nksr_splat_keys / nksr_cell_footprint_keys / nksr_cell_corner_keys on a 3 000-point sphere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -0x0123456789ABCDEF
BATCH, RANGE = 2048, 4 * 2048          # mode 3: keys of a batch, keys of a workgroup's range (streams of fewer than 8192 batches)


def _dev():
    return torch.device('cuda:0')


def _run(xyz, cells, n, inv_w0, level, mode, per):
    """one call; returns the keys written.  Checks the count against the capacity and the guard words behind keys_out."""
    from nksr_amd._lib import call, ptr, stream
    cap = n * per
    out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int64, device=_dev())
    cnt = torch.full((1,), -5, dtype=torch.int64, device=_dev())
    call('nksr_footprint_keys_dedup', ptr(xyz) if xyz is not None else None, ptr(cells) if cells is not None else None, n,
         float(inv_w0), level, mode, ptr(out), ptr(cnt), stream())
    torch.cuda.synchronize()
    c = int(cnt.cpu().numpy()[0])
    assert 0 <= c <= cap, 'count %d outside [0, %d]' % (c, cap)
    assert bool((out[cap:] == SENTINEL).all()), 'guard words behind keys_out were written'
    assert bool((out[c:cap] == SENTINEL).all()), 'keys written past the count'
    return out[:c].cpu().numpy()


def _check(tag, stream_np, run):
    """the contract, for one stream: same key set, unique count <= count <= length, twice the same sorted-unique result"""
    want = np.unique(stream_np)
    a, b = run(), run()
    print('%s: %d keys, %d distinct, %d / %d written' % (tag, stream_np.size, want.size, a.size, b.size))
    assert want.size <= a.size <= stream_np.size, '%s: %d keys written, %d distinct of %d' % (tag, a.size, want.size, stream_np.size)
    assert set(a.tolist()) == set(want.tolist()), tag + ': the key set differs'
    assert np.array_equal(np.unique(a), np.unique(b)), tag + ': two runs differ'
    return a.size


def _distinct(n, seed=0):
    """n distinct non-negative keys in random order, spread over 40 bits"""
    rs = np.random.RandomState(seed)
    return (rs.permutation(n).astype(np.int64) * 1000003 + 17) % (1 << 40) + (rs.randint(0, 1 << 20) << 40)


def _streams():
    S = {'one': _distinct(1)}
    for n in (BATCH - 1, BATCH, BATCH + 1):
        S['distinct%d' % n] = _distinct(n, n)
    S['distinct_every_batch_flushes'] = _distinct(5 * BATCH + 7, 3)
    S['one_key_40000_times'] = np.full(40000, 123456789012, np.int64)
    S['each_key_three_times'] = np.repeat(_distinct(5000, 4), 3)
    S['cycle_1500_x30'] = np.tile(_distinct(1500, 5), 30)
    for n in (RANGE - 1, RANGE, RANGE + 1):
        S['range%d' % n] = np.repeat(_distinct((n + 2) // 3, n), 3)[:n]
    return S


STREAMS = _streams()


@pytest.mark.parametrize('name', sorted(STREAMS))
def test_mode3_streams_keep_their_key_set(name):
    s = STREAMS[name]
    assert len(np.unique(s)) >= 1 and s.min() >= 0
    keys = torch.from_numpy(s).to(_dev())
    written = _check(name, s, lambda: _run(None, keys, s.size, 0.0, 0, 3, 1))
    if name == 'one_key_40000_times':
        # 20 batches = 5 ranges of 4: a set that lives through its range emits the key once per RANGE, not once per batch
        assert written == -(-s.size // RANGE), written
    if name == 'each_key_three_times':
        # a batch brings ~683 new keys: the set takes two batches (<= 1024 occupied before the second), so a key's three copies
        # meet in it unless a flush or the end of a range falls between them -- at most once per two batches
        assert written <= 5000 + 2 * (-(-s.size // (2 * BATCH))), written


def test_the_python_wrapper_returns_the_same_set():
    from nksr_amd import ops
    s = STREAMS['cycle_1500_x30']
    got = ops.dedup_keys(torch.from_numpy(s).to(_dev())).cpu().numpy()
    assert set(got.tolist()) == set(np.unique(s).tolist()) and got.size <= s.size


def test_empty_stream_writes_nothing_and_counts_zero():
    keys = torch.zeros(1, dtype=torch.int64, device=_dev())
    assert _run(None, keys, 0, 0.0, 0, 3, 1).size == 0
    xyz = torch.zeros((1, 3), dtype=torch.float32, device=_dev())
    assert _run(xyz, None, 0, 10.0, 0, 0, 8).size == 0


@pytest.fixture(scope='module')
def sphere():
    """a 3 000-point sphere in Morton order, its point keys and the unique cells of every level"""
    from nksr_amd import utils
    from nksr_amd.nn.network import sort_cloud
    from nksr_amd.svh import SparseFeatureHierarchy, inv_w0_f32
    xyz, _ = utils.synth_sphere(3000, 0.45, 0.003, seed=1)
    x = torch.from_numpy(xyz).to(_dev())
    inv_w0 = inv_w0_f32(0.02)
    ks, xs, _ = sort_cloud(x.contiguous(), x.contiguous(), inv_w0)
    cells = SparseFeatureHierarchy.cells_with_points(ks, 3)
    return xs.contiguous(), inv_w0, [c.contiguous() for c in cells]


def _plain(fn, *args, n, per):
    from nksr_amd._lib import call, ptr, stream
    raw = torch.empty(n * per, dtype=torch.int64, device=_dev())
    call(fn, *args, ptr(raw), stream())
    torch.cuda.synchronize()
    return raw.cpu().numpy()


@pytest.mark.parametrize('mode,level', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_point_footprints_against_the_plain_stream(sphere, mode, level):
    from nksr_amd._lib import ptr
    xs, inv_w0, _ = sphere
    n, per = xs.shape[0], 8 if mode == 0 else 27
    plain = _plain('nksr_splat_keys', ptr(xs), n, inv_w0, level, mode, n=n, per=per)
    _check('points mode %d level %d' % (mode, level), plain, lambda: _run(xs, None, n, inv_w0, level, mode, per))


@pytest.mark.parametrize('mode,level', [(0, 0), (0, 1), (1, 0), (1, 2)])
def test_cell_footprints_against_the_plain_stream(sphere, mode, level):
    from nksr_amd._lib import ptr
    _, inv_w0, cells = sphere
    c = cells[level]
    n, per = c.numel(), 8 if mode == 0 else 27
    plain = _plain('nksr_cell_footprint_keys', ptr(c), n, level, mode, n=n, per=per)
    _check('cells mode %d level %d' % (mode, level), plain, lambda: _run(None, c, n, inv_w0, level, mode, per))


def test_cell_corners_against_the_plain_stream(sphere):
    from nksr_amd._lib import ptr
    _, inv_w0, cells = sphere
    c = cells[0]
    plain = _plain('nksr_cell_corner_keys', ptr(c), c.numel(), n=c.numel(), per=8)
    _check('corners', plain, lambda: _run(None, c, c.numel(), inv_w0, 0, 2, 8))
