"""The numpy restatement of the mesh rasteriser (tests/mesh_raster_ref.py) against analytic cases -- it has to earn its place as the
yardstick of tests/test_gpu_mesh_raster.py -- and what needs no GPU: the argument errors, the C ABI's argument checks, the wiring and the
ASCII grid writer."""
import numpy as np
import pytest

import mesh_raster_ref as R

EPS = np.finfo(np.float64).eps


def test_tilted_plane_gives_the_plane_at_the_centres():
    a, b, c = 0.37, -1.21, 5.5
    xy = np.array([[-1.3, -0.7], [9.1, -0.9], [8.7, 7.9], [-0.8, 8.3]])
    v = np.concatenate([xy, (a * xy[:, :1] + b * xy[:, 1:] + c)], 1)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    for surface in ('top', 'bottom'):
        hm = R.height_map(v, f, 0.5, origin=(0.0, 0.0), shape=(15, 14), surface=surface)
        X, Y = R.centres(0.0, 0.5, 15)[:, None], R.centres(0.0, 0.5, 14)[None, :]
        assert np.all(hm['count'] == 1) and set(np.unique(hm['face'])) == {0, 1}
        err = np.abs(hm['height'] - (a * X + b * Y + c)).max()
        print('tilted plane (%s): largest error %.3g of bound %.3g' % (surface, err, 8 * EPS * np.abs(v[:, 2]).max()))
        assert err <= 8 * EPS * np.abs(v[:, 2]).max()
    # the other five axis orders see the same plane through their own frame
    hm = R.height_map(v[:, [2, 0, 1]], f, 0.5, origin=(0.0, 0.0), shape=(15, 14), axes=(1, 2))
    assert np.array_equal(hm['height'], R.height_map(v, f, 0.5, origin=(0.0, 0.0), shape=(15, 14))['height'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('offset', [0.0, 1e6])
def test_snapped_icosphere_has_even_counts(dtype, offset):
    v, f = R.snapped_icosphere(1.0, 11.0, offset, dtype)
    hm = R.height_map(v, f, 1.0, origin=(offset - 12.0, offset - 12.0), shape=(24, 24))
    X = R.centres(offset - 12.0, 1.0, 24)
    on_centre = np.isin(v[:, 0].astype(np.float64), X) & np.isin(v[:, 1].astype(np.float64), X)
    print('icosphere %s at %g: %d vertices under a centre, counts %s' % (np.dtype(dtype).name, offset, on_centre.sum(), np.unique(hm['count'])))
    assert on_centre.sum() >= 32                                 # the case is what it claims to be: vertices exactly under centres
    assert np.all(hm['count'] % 2 == 0) and hm['count'].max() == 2 and (hm['count'] == 2).sum() > 300
    bottom = R.height_map(v, f, 1.0, origin=(offset - 12.0, offset - 12.0), shape=(24, 24), surface='bottom')
    covered = hm['count'] > 0
    assert np.array_equal(bottom['count'], hm['count']) and np.all(hm['height'][covered] >= bottom['height'][covered])


@pytest.mark.parametrize('mixed', [False, True])
def test_diagonal_square_is_claimed_once_and_its_border_is_half_open(mixed):
    v, f = R.diagonal_square(6, 1.0, mixed)
    # centres on the diagonal and, with the origin shifted by half a pixel, on the border: pixel k has its centre at k
    hm = R.height_map(v, f, 1.0, origin=(0.0, 0.0), shape=(6, 6))
    assert np.all(hm['count'] == 1) and hm['n_hits'] == 36
    hm = R.height_map(v, f, 1.0, origin=(-1.5, -1.5), shape=(9, 9))
    inside = np.zeros((9, 9), bool)
    inside[1:7, 1:7] = True                                      # centres 0 .. 5 of -1 .. 7: the low border in, the high border (6) out
    assert np.array_equal(hm['count'], inside.astype(np.int32))
    assert np.array_equal(np.diff(hm['pixel_start']), hm['count'].reshape(-1)) and np.array_equal(hm['face'] >= 0, inside)


def test_neighbouring_tiles_claim_every_border_pixel_once():
    # two squares that share the edge x = 3, each cut along a diagonal, the right one wound the other way
    v = np.array([[0, 0, 0], [3, 0, 0], [3, 3, 0], [0, 3, 0], [6, 0, 1], [6, 3, 1]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [1, 5, 4], [1, 2, 5]])
    hm = R.height_map(v, f, 1.0, origin=(-0.5, -0.5), shape=(7, 4))
    assert np.array_equal(hm['count'], np.concatenate([np.ones((6, 3), np.int32), np.zeros((6, 1), np.int32)], 1).tolist() + [[0, 0, 0, 0]])


def test_layers_vertical_faces_dropped_faces_and_ties():
    v = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1], [0, 0, 3], [4, 0, 3], [0, 4, 3], [1, 1, 0], [1, 1, 5], [3, 1, 2], [np.nan, 0, 0]], np.float64)
    f = np.array([[3, 4, 5], [0, 1, 2], [6, 7, 8], [0, 1, 99], [0, 1, 9], [0, 2, 1], [-1, 0, 1]])
    hm = R.height_map(v, f, 1.0, origin=(0.0, 0.0), shape=(4, 4))
    assert hm['n_dropped'] == 3                                  # an index past the end, a NaN corner, a negative index
    assert hm['count'][0, 0] == 3 and hm['height'][0, 0] == 3.0 and hm['face'][0, 0] == 0
    s = hm['pixel_start']
    assert hm['layer_face'][s[0]:s[1]].tolist() == [0, 1, 5] and hm['layer_height'][s[0]:s[1]].tolist() == [3.0, 1.0, 1.0]
    assert not np.any(hm['layer_face'] == 2)                     # the wall x in [1, 3], y = 1 is vertical: it covers nothing
    bottom = R.height_map(v, f, 1.0, origin=(0.0, 0.0), shape=(4, 4), surface='bottom')
    assert bottom['height'][0, 0] == 1.0 and bottom['face'][0, 0] == 1         # faces 1 and 5 tie: the lower id
    assert hm['count'][3, 3] == 0 and np.isnan(hm['height'][3, 3]) and hm['face'][3, 3] == -1
    # origin=None and shape=None: the lattice point at or below the minimum, up to the maximum
    hm = R.height_map(v + 0.25, f, 0.5)
    assert hm['origin'] == (0.0, 0.0) and hm['shape'] == (9, 9)


def test_gradient_and_hillshade_of_a_plane():
    p = 0.5
    X, Y = R.centres(0.0, p, 7)[:, None], R.centres(0.0, p, 6)[None, :]
    h = 0.25 * X - 0.5 * Y + 1.0                                  # dyadic: exact
    h[4, 4] = np.nan
    gx, gy = R.gradient(h, p)
    inner = np.zeros(h.shape, bool)
    inner[1:-1, 1:-1] = True
    inner[3:6, 3:6] = False                                      # beside the hole
    assert np.all(np.isnan(gx[~inner])) and np.all(np.isnan(gy[~inner]))
    assert np.all(gx[inner] == 0.25) and np.all(gy[inner] == -0.5)
    s = R.sun(315.0, 45.0)
    assert abs(np.linalg.norm(s) - 1.0) < 4 * EPS and s[0] < 0 < s[1] and s[2] > 0          # from the north-west, above the horizon
    shade = R.hillshade(h, p)
    want = (s[2] - (s[0] * 0.25 + s[1] * -0.5)) / np.sqrt(1.0 + 0.25 ** 2 + 0.5 ** 2)
    assert np.all(np.abs(shade[inner] - want) < 4 * EPS) and np.all(np.isnan(shade[~inner]))
    assert np.all(R.hillshade(h, p, 135.0, 5.0)[inner] == 0.0)                              # lit from behind: clamped


def test_argument_errors_need_no_gpu():
    from nksr_amd import mesh_raster as mr
    ext = (0.0, 10.0, -5.0, 5.0)
    assert mr.raster_grid(0.5, None, None, ext) == (0.5, (0.0, -5.0), (21, 21))
    assert mr.raster_grid(0.5, (1.0, 2.0), (3, 4), None) == (0.5, (1.0, 2.0), (3, 4))
    assert mr.raster_grid(1.0, None, None, None) == (1.0, (0.0, 0.0), (0, 0))
    for bad in (0.0, -1.0, float('nan'), float('inf'), 'wide', None):
        with pytest.raises(ValueError):
            mr.raster_grid(bad, None, None, ext)
    with pytest.raises(ValueError, match='2\\^-40'):
        mr.raster_grid(1e-7, None, None, (0.0, 1e6, 0.0, 1.0))                  # 2^-40 of 1e6 is 9.1e-7
    with pytest.raises(ValueError, match='2\\^-40'):
        mr.raster_grid(1e-7, (1e6, 0.0), (4, 4), (0.0, 1.0, 0.0, 1.0))          # the origin counts too
    assert mr.raster_grid(1e-6, None, (4, 4), (0.0, 1e6, 0.0, 1.0))[0] == 1e-6
    with pytest.raises(ValueError, match='2\\^31'):
        mr.raster_grid(1.0, (0.0, 0.0), (1 << 16, 1 << 15), ext)
    assert mr.raster_grid(1.0, (0.0, 0.0), ((1 << 16) - 1, 1 << 15), ext)[2] == ((1 << 16) - 1, 1 << 15)
    with pytest.raises(ValueError, match='2\\^31'):
        mr.raster_grid(1e-4, None, None, ext)                                    # 100001 x 100001 pixels
    for bad in ((0.0,), (0.0, float('nan')), 'ab', 3):
        with pytest.raises(ValueError):
            mr.raster_grid(1.0, bad, (2, 2), ext)
    for bad in ((2,), (2, -1), (2.0, 2), (True, 2), 5):
        with pytest.raises(ValueError):
            mr.raster_grid(1.0, (0.0, 0.0), bad, ext)
    assert mr.raster_axes((0, 1)) == (0, 1, 2) and mr.raster_axes([2, 0]) == (2, 0, 1) and mr.raster_axes((1, 2)) == (1, 2, 0)
    for bad in ((0, 0), (0, 3), (0,), (0, 1, 2), (True, 0), (0.0, 1), 1, None):
        with pytest.raises(ValueError):
            mr.raster_axes(bad)
    assert mr.raster_surface('top') == 'top' and mr.raster_surface('bottom') == 'bottom'
    for bad in ('up', None, 0):
        with pytest.raises(ValueError):
            mr.raster_surface(bad)
    assert np.array_equal(mr.sun_vector(315.0, 45.0), R.sun(315.0, 45.0))
    with pytest.raises(ValueError):
        mr.sun_vector(float('nan'), 45.0)


def test_raster_c_abi_argument_errors_without_a_gpu():
    import ctypes as C
    from nksr_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    A, Z = C.cast(buf, C.c_void_p), None

    def err():
        return lib.nksr_last_error().decode()

    assert lib.nksr_raster_boxes(A, 1, 3, A, 0, 1, 0, 0, 0.0, 0.0, 1.0, 4, 4, A, A, A, Z) != 0 and 'axes' in err()
    assert lib.nksr_raster_boxes(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 0.0, 4, 4, A, A, A, Z) != 0 and 'pixel' in err()
    assert lib.nksr_raster_boxes(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 1.0, 1 << 16, 1 << 15, A, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_raster_boxes(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 1.0, 4, 4, A, Z, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_boxes(A, 1, 3, A, 0, -1, 0, 1, 0.0, 0.0, 1.0, 4, 4, A, A, A, Z) != 0 and 'negative' in err()
    assert lib.nksr_raster_test(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 1.0, 4, 4, A, A, 1 << 31, A, A, Z) != 0 and '2^31' in err()
    assert lib.nksr_raster_test(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 1.0, 4, 4, A, A, 5, Z, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_test(A, 1, 3, A, 0, 0, 0, 1, 0.0, 0.0, 1.0, 4, 4, A, A, 5, A, A, Z) != 0 and 'without faces' in err()
    assert lib.nksr_raster_test(Z, 1, 0, Z, 0, 0, 0, 1, 0.0, 0.0, 1.0, 4, 4, Z, Z, 0, Z, Z, Z) == 0
    assert lib.nksr_raster_flag_counts(Z, 5, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_compact(A, A, A, A, 1, 5, 4, 4, A, 6, A, A, A, Z) != 0 and 'hits' in err()
    assert lib.nksr_raster_compact(A, A, A, A, 1, 5, 4, 4, A, 2, A, Z, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_compact(Z, Z, Z, Z, 0, 0, 4, 4, Z, 0, Z, Z, Z, Z) == 0
    assert lib.nksr_raster_pixel_start(A, A, 3, 2, 16, A, Z) != 0 and 'runs' in err()
    assert lib.nksr_raster_pixel_start(A, A, 2, 2, 16, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_reduce(A, A, 2, A, A, A, 2, 0, 16, A, A, A, A, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_reduce(A, A, 2, A, A, A, 2, 0, 1, A, A, A, A, A, Z) != 0 and 'runs' in err()
    assert lib.nksr_raster_reduce(Z, Z, 0, Z, Z, Z, 0, 0, 16, Z, Z, Z, Z, Z, Z) == 0
    assert lib.nksr_raster_sample(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 1.0, 4, 4, A, A, 1, -1, A, Z) != 0 and 'channels' in err()
    assert lib.nksr_raster_sample(A, 1, 3, A, 0, 1, 0, 1, 0.0, 0.0, 1.0, 4, 4, Z, A, 1, 3, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_horn(A, 4, 4, 1.0, Z, A, A, A, Z) != 0 and 'NULL' in err()
    assert lib.nksr_raster_horn(A, 4, 4, -1.0, A, A, A, A, Z) != 0 and 'pixel' in err()
    assert lib.nksr_raster_horn(Z, 0, 4, 1.0, A, Z, Z, Z, Z) == 0


def test_mesh_rasterizer_is_exported_and_documented():
    import nksr
    from nksr_amd import _lib, build, mesh_raster
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_raster import HeightMap, MeshRasterizer
    assert 'MeshRasterizer' in nksr.__all__ and nksr.MeshRasterizer is MeshRasterizer and nksr.metrics.MeshRasterizer is MeshRasterizer
    assert 'meshraster.hip' in build.SOURCES
    assert callable(MeshingResult.height_map) and callable(MeshRasterizer.height_map)
    assert all(callable(getattr(HeightMap, name)) for name in ('layers', 'sample', 'gradient', 'slope', 'hillshade'))
    for name in ('boxes', 'test', 'flag_counts', 'compact', 'pixel_start', 'reduce', 'sample', 'horn'):
        assert 'nksr_raster_' + name in _lib.EXPORTED and hasattr(_lib.lib, 'nksr_raster_' + name), name
    assert 'bit for bit' in mesh_raster.__doc__ and 'atomic' in mesh_raster.__doc__ and _lib.RASTER_BLOCK == 256


def test_write_ascii_grid_round_trips_north_up(tmp_path):
    from nksr_amd import utils
    h = np.arange(12, dtype=np.float64).reshape(4, 3) / 7.0             # [nx = 4, ny = 3]
    h[1, 2] = np.nan
    path = str(tmp_path / 'dem.asc')
    utils.write_ascii_grid(path, h, (100.5, -20.25), 0.5)
    with open(path) as fh:
        head = [fh.readline().split() for _ in range(6)]
    assert [k for k, _ in head] == ['ncols', 'nrows', 'xllcorner', 'yllcorner', 'cellsize', 'NODATA_value']
    assert [float(x) for _, x in head] == [4.0, 3.0, 100.5, -20.25, 0.5, -9999.0]
    rows = np.loadtxt(path, skiprows=6)
    assert rows.shape == (3, 4)
    back = rows[::-1].T                                          # the first row is the largest j
    assert np.array_equal(back[~np.isnan(h)], h[~np.isnan(h)]) and back[1, 2] == -9999.0
    assert np.array_equal(rows[0], np.where(np.isnan(h[:, 2]), -9999.0, h[:, 2]))
    utils.write_ascii_grid(path, h, (0.0, 0.0), 2.0, nodata=-1.0)
    assert np.loadtxt(path, skiprows=6)[0, 1] == -1.0
    with pytest.raises(ValueError):
        utils.write_ascii_grid(path, h.reshape(-1), (0.0, 0.0), 1.0)
    with pytest.raises(ValueError):
        utils.write_ascii_grid(path, h, (0.0, 0.0), 0.0)
