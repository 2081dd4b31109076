"""The host side of the chunk path (nksr_amd/chunking/geometry.py, driver.py) on its own, no GPU: the exploded frame against the
oracle's statement of it (oracle/chunking.py: Frame), the one chunk-index routine against the oracle's chunk ids and a plain loop,
the greedy batch plan on hand-written cases, and the names the package exports."""
import math
import types

import numpy as np
import pytest
import torch

# (voxel_size, tree_depth, lo, grid, chunk_size, overlap_ratio)
SETUPS = [(0.1, 4, [-3.3, 0.2, 1.0], [3, 2, 1], 12.5, 0.05),
          (0.25, 5, [-500.0, -500.0, 0.0], [8, 8, 1], 125.0, 0.05),
          (0.02, 3, [0.0, 0.0, 0.0], [1, 1, 1], 4.0, 0.1),
          (0.1, 5, [-7.7, 3.1, -2.2], [2, 3, 4], 9.0, 0.2)]


@pytest.mark.parametrize('voxel_size,depth,lo,grid,chunk_size,overlap', SETUPS)
def test_chunk_frame_equals_the_oracle_frame(voxel_size, depth, lo, grid, chunk_size, overlap):
    from nksr_amd import chunking
    from oracle import chunking as oc
    ov, band = chunking.chunk_geometry(types.SimpleNamespace(voxel_size=voxel_size, tree_depth=depth), chunk_size, overlap)
    frame = chunking.ChunkFrame(voxel_size, depth, lo, grid, chunk_size, band)
    ref = oc.Frame(voxel_size, depth, lo, grid, chunk_size, band)
    assert frame.S == ref.S
    ranges = []
    for c in range(grid[0] * grid[1] * grid[2]):
        assert tuple(frame.chunk3(c)) == tuple(ref.c3(c))
        assert (frame.chunk3(c)[0] * grid[1] + frame.chunk3(c)[1]) * grid[2] + frame.chunk3(c)[2] == c
        assert list(frame.shift_cells(c)) == list(ref.shift_cells(c))
        a, b = frame.shift(c), ref.shift(c)
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
        ranges.append(frame.key_range(c))
    # a slot is an aligned cube of the Morton lattice: one key range of 8^S keys starting at a multiple of 8^S, no two alike
    size = 1 << (3 * frame.S)
    assert all(hi - lo_ == size and lo_ % size == 0 for lo_, hi in ranges)
    assert len({lo_ for lo_, _ in ranges}) == len(ranges)


def _face_points(lo, grid, chunk_size, seed):
    """Random points in the box grown by a tenth + points exactly on, one ulp below and one ulp above every chunk face (the outer
    faces included: beyond them a point clamps to the border chunk)."""
    rs = np.random.RandomState(seed)
    lo_a = np.asarray(lo)
    ext = np.asarray(grid) * chunk_size
    pts = [rs.uniform(-0.1, 1.1, (3000, 3)) * ext + lo_a]
    for a in range(3):
        for j in range(grid[a] + 1):
            f = np.float32(lo[a] + j * chunk_size)
            for v in (f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
                p = pts[0][:16].copy()
                p[:, a] = v
                pts.append(p)
    return np.concatenate(pts).astype(np.float32)


@pytest.mark.parametrize('lo,grid,chunk_size', [(s[2], s[3], s[4]) for s in (SETUPS[0], SETUPS[3])])
def test_chunk_index_equals_the_oracle_a_plain_loop_and_its_callers(lo, grid, chunk_size):
    from nksr_amd import chunking
    from nksr_amd.chunking import driver
    from oracle import chunking as oc
    xyz = _face_points(lo, grid, chunk_size, 5)
    xt = torch.from_numpy(xyz)
    idx, cid = chunking.chunk_index(xt, lo, grid, chunk_size)
    cid = cid.numpy()
    assert np.array_equal(cid, oc.chunk_ids(xyz, lo, chunk_size, grid))
    loop = np.zeros(len(xyz), np.int64)
    for i, p in enumerate(xyz):
        i3 = [min(max(int(math.floor((p[a] - np.float32(lo[a])) / np.float32(chunk_size))), 0), grid[a] - 1) for a in range(3)]      # fp32 throughout
        loop[i] = (i3[0] * grid[1] + i3[1]) * grid[2] + i3[2]
        assert [int(idx[a][i]) if grid[a] > 1 else idx[a] for a in range(3)] == i3
    assert np.array_equal(cid, loop)
    assert cid.min() == 0 and cid.max() == grid[0] * grid[1] * grid[2] - 1 and len(np.unique(cid)) == grid[0] * grid[1] * grid[2]
    # an offset moves the point, not the grid
    off = 0.3 * chunk_size
    assert torch.equal(chunking.chunk_index(xt, lo, grid, chunk_size, off)[1], chunking.chunk_index(xt + off, lo, grid, chunk_size)[1])
    # the blended field and the driver ask the same routine
    field = types.SimpleNamespace(origin=lo, grid=grid, chunk_size=float(chunk_size))
    assert np.array_equal(chunking.MultiChunkField.chunk_of(field, xt).numpy(), cid)
    hp = types.SimpleNamespace(voxel_size=0.1, tree_depth=4)
    hi = [lo[a] + grid[a] * chunk_size for a in range(3)]
    plan = driver.chunk_plan(hp, xt, lo, hi, chunk_size, 0.05, 0, 1, False, False, None)
    assert plan.grid == grid and plan.counts == np.bincount(cid, minlength=plan.nchunk).tolist()
    assert plan.jobs == list(range(plan.nchunk)) and plan.owner == [0] * plan.nchunk
    for c in range(plan.nchunk):
        c3 = plan.frame.chunk3(c)
        assert plan.cores[c] == ([lo[a] + c3[a] * chunk_size for a in range(3)], [lo[a] + c3[a] * chunk_size + chunk_size for a in range(3)])


def test_batch_plan_on_hand_written_cases():
    from nksr_amd.chunking import plan_batches
    npts = {0: 10, 1: 20, 2: 30, 3: 40, 7: 5}
    assert plan_batches([], npts, 100) == []
    assert plan_batches([], npts, 0) == []
    assert plan_batches([3, 0, 7, 1], npts, 0) == [[3], [0], [7], [1]]                  # budget 0: one chunk per batch
    assert plan_batches([0, 3, 1], npts, 35) == [[0], [3], [1]]                          # 40 > 35: alone, and it closes the batch before it
    assert plan_batches([3, 0, 1], npts, 35) == [[3], [0, 1]]
    assert plan_batches([0, 1, 2], npts, 60) == [[0, 1, 2]]                              # 10 + 20 + 30: an exact fit stays together
    assert plan_batches([0, 1, 2], {0: 10, 1: 20, 2: 31}, 60) == [[0, 1], [2]]           # one point more splits
    assert plan_batches([2, 7, 1, 0, 3], npts, 55) == [[2, 7, 1], [0, 3]]                # the order of the jobs is the order of the batches
    assert plan_batches([0, 1, 2, 3, 7], npts, 1 << 25) == [[0, 1, 2, 3, 7]]


def test_public_surface_of_the_package():
    from nksr_amd import chunking
    names = ('reconstruct_by_chunk select_chunk_points chunk_grid chunk_geometry chunk_grid_struct ChunkFrame ChunkPart MultiChunkField '
             'ChunkUnionMask ChunkTooSmall pack_field unpack_field fields_from_payloads exchange_band halo_inner halo_destinations '
             'needed_chunks borrowed spill_to_disk OV_FLOOR BAND_EXTRA MIN_CHUNK_POINTS SLOT_GAP').split()
    assert [n for n in names if not hasattr(chunking, n)] == []
