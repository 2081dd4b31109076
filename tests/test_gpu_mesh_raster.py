"""The GPU mesh rasteriser (nksr_amd/mesh_raster.py, csrc/meshraster.hip) against its numpy restatement (tests/mesh_raster_ref.py), which
is a brute force over every (face, pixel) pair: every array in full, integers index for index with their dtype, heights, layers,
gradients and shades bit for bit.  Every comparison prints its largest error before it asserts."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_raster_ref as R

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOUP = dict(pixel=0.25, origin=(-3.0, -2.0), shape=(37, 29))


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same_ints(name, got, want, dtype):
    got, want = _host(got), np.asarray(want)
    assert got.dtype == dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    diff = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max(initial=0))
    print('%s: %s, largest difference %d' % (name, got.shape, diff))
    assert np.array_equal(got, want.astype(dtype)), name


def _same_bits(name, got, want):
    got, want = _host(got), np.asarray(want, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), name + ': the empty pixels differ'
    err = float(np.abs(got[~nan] - want[~nan]).max(initial=0.0))
    print('%s: %s, %d values, largest error %.3g' % (name, got.shape, int((~nan).sum()), err))
    assert np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)), name


def _same_map(label, hm, ref):
    """Every array of a HeightMap against the restatement's."""
    assert hm.shape == ref['shape'] and hm.origin == ref['origin'] and hm.pixel_size == ref['pixel_size'], (label, hm.shape, hm.origin, ref['shape'], ref['origin'])
    assert (hm.n_dropped, hm.n_hits) == (ref['n_dropped'], ref['n_hits']), (label, hm.n_dropped, hm.n_hits, ref['n_dropped'], ref['n_hits'])
    start, layer_face, layer_height = hm.layers()
    _same_ints(label + ' count', hm.count, ref['count'], np.int32)
    _same_ints(label + ' face', hm.face, ref['face'], np.int32)
    _same_bits(label + ' height', hm.height, ref['height'])
    _same_ints(label + ' pixel_start', start, ref['pixel_start'], np.int64)
    _same_ints(label + ' layer_face', layer_face, ref['layer_face'], np.int32)
    _same_bits(label + ' layer_height', layer_height, ref['layer_height'])
    assert np.array_equal(_host(hm.valid), ref['count'] > 0) and hm.valid.dtype == torch.bool


def _rasterizer(v, f, attr=None):
    from nksr_amd.mesh_raster import MeshRasterizer
    return MeshRasterizer(v, f, attr)


@functools.lru_cache(maxsize=None)
def _soup(dtype):
    v, f = R.triangle_soup(300, *SOUP['shape'], SOUP['pixel'], SOUP['origin'], dtype=dtype)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def _soup_ref(dtype, surface='top'):
    v, f = _soup(dtype)
    return R.height_map(v, f, SOUP['pixel'], SOUP['origin'], SOUP['shape'], surface=surface)


def _soup_map(v, f, **kw):
    return _rasterizer(v, f).height_map(SOUP['pixel'], SOUP['origin'], SOUP['shape'], **kw)


# ---- triangle soup ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('as_torch', [False, True], ids=['numpy', 'torch'])
@pytest.mark.parametrize('itype', [np.int32, np.int64], ids=['int32', 'int64'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
def test_triangle_soup_equals_the_restatement(dtype, itype, as_torch):
    v, f = _soup(dtype)
    ref = _soup_ref(dtype)
    vv, ff = v.copy(), f.astype(itype)
    if as_torch:
        vv, ff = torch.from_numpy(vv), torch.from_numpy(ff).cuda()           # a host tensor and a device tensor
    hm = _soup_map(vv, ff)
    print('soup: %d candidates, %d hits, largest count %d, %d empty pixels' % (hm.n_candidates, hm.n_hits, int(hm.count.max()), int((hm.count == 0).sum())))
    assert hm.n_candidates > 256 * 8 and hm.n_faces == 300 and ref['n_hits'] > 1000 and ref['count'].max() >= 3 and (ref['count'] == 0).any()
    _same_map('soup', hm, ref)
    assert (hm.axes, hm.up, hm.surface) == ((0, 1), 2, 'top')


@pytest.mark.parametrize('axes', [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)])
def test_triangle_soup_in_every_axis_order(axes):
    v, f = _soup(np.float64)
    up = 3 - axes[0] - axes[1]
    w = np.empty_like(v)
    w[:, axes[0]], w[:, axes[1]], w[:, up] = v[:, 0], v[:, 1], v[:, 2]
    hm = _soup_map(w, f.astype(np.int32), axes=axes)
    assert (hm.axes, hm.up) == (axes, up)
    _same_map('soup axes %s' % (axes,), hm, _soup_ref(np.float64))
    _same_map('soup axes %s restated' % (axes,), hm, R.height_map(w, f, SOUP['pixel'], SOUP['origin'], SOUP['shape'], axes=axes))


def test_bottom_surface_of_the_soup():
    v, f = _soup(np.float64)
    top, bottom = _soup_ref(np.float64), _soup_ref(np.float64, 'bottom')
    hm = _soup_map(v, f, surface='bottom')
    _same_map('soup bottom', hm, bottom)
    covered = top['count'] > 0
    assert np.all(top['height'][covered] >= bottom['height'][covered]) and (top['face'] != bottom['face']).any()


# ---- closed mesh --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0.0, 1e6])
def test_snapped_icosphere_has_even_counts(offset):
    v, f = R.snapped_icosphere(1.0, 11.0, offset)
    assert len(f) == 320
    grid = dict(pixel_size=1.0, origin=(offset - 12.0, offset - 12.0), shape=(24, 24))
    r = _rasterizer(v, f)
    top, bottom = r.height_map(**grid), r.height_map(surface='bottom', **grid)
    _same_map('icosphere top', top, R.height_map(v, f, **grid))
    _same_map('icosphere bottom', bottom, R.height_map(v, f, surface='bottom', **grid))
    count = _host(top.count)
    print('icosphere at %g: counts %s' % (offset, np.unique(count)))
    assert np.all(count % 2 == 0) and count.max() == 2 and (count == 2).sum() > 300
    covered = count > 0
    assert np.all(_host(top.height)[covered] >= _host(bottom.height)[covered])


# ---- large faces, deep stacks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mixed', [False, True], ids=['equal', 'mixed'])
def test_two_large_faces_share_their_diagonal(mixed):
    v, f = R.diagonal_square(300, 1.0, mixed)
    v[:, 2] = [0.0, 1.0, 3.0, 2.0]
    hm = _rasterizer(v, f).height_map(1.0, origin=(0.0, 0.0), shape=(300, 300))
    assert hm.n_candidates == 2 * 300 * 300 and 300 * 300 > 1 << 16         # one face, more than 2^16 candidates, across many blocks
    assert bool((hm.count == 1).all()) and hm.n_hits == 300 * 300
    _same_map('large faces', hm, R.height_map(v, f, 1.0, origin=(0.0, 0.0), shape=(300, 300)))


def test_a_stack_deeper_than_a_wavefront():
    v = np.array([[-10, -10, 1], [30, -10, 2], [-10, 30, 3]], np.float32)
    f = np.tile(np.array([[0, 1, 2]], np.int32), (100, 1))
    hm = _rasterizer(v, f).height_map(1.0, origin=(0.0, 0.0), shape=(5, 5))
    assert bool((hm.count == 100).all()) and bool((hm.face == 0).all()) and hm.n_hits == 2500
    start, layer_face, layer_height = hm.layers()
    assert np.array_equal(_host(start), np.arange(26) * 100)
    assert np.array_equal(_host(layer_face).reshape(25, 100), np.tile(np.arange(100), (25, 1)))           # ascending face id per pixel
    assert np.array_equal(_host(layer_height).reshape(25, 100), np.repeat(_host(hm.height).reshape(25, 1), 100, 1))
    _same_map('deep stack', hm, R.height_map(v, f, 1.0, origin=(0.0, 0.0), shape=(5, 5)))


# ---- order and repeats --------------------------------------------------------------------------------------------------------------
def test_face_order_does_not_change_the_rasters():
    v, f = _soup(np.float64)
    ref = _soup_ref(np.float64)
    perm = np.random.default_rng(11).permutation(len(f))
    hm = _soup_map(v, f[perm])
    _same_bits('shuffled height', hm.height, ref['height'])
    _same_ints('shuffled count', hm.count, ref['count'], np.int32)
    # wherever exactly one layer attains the best height the face maps back through the permutation
    start, best = ref['pixel_start'], ref['height'].reshape(-1)
    attained = np.array([np.count_nonzero(ref['layer_height'][start[k]:start[k + 1]] == best[k]) for k in range(len(best))]).reshape(ref['shape'])
    once = attained == 1
    print('shuffled: the best height is attained once on %d of %d covered pixels' % (once.sum(), (ref['count'] > 0).sum()))
    assert once.sum() > 300 and np.array_equal(perm[_host(hm.face)[once]], ref['face'][once])


def test_two_calls_give_the_same_bits():
    v, f = _soup(np.float32)
    attr = np.random.default_rng(2).normal(size=(len(v), 3)).astype(np.float32)
    runs = []
    for _ in range(2):
        hm = _rasterizer(v, f, attr).height_map(SOUP['pixel'], SOUP['origin'], SOUP['shape'])
        runs.append([hm.height, hm.face, hm.count, *hm.layers(), hm.sample(), *hm.gradient(), hm.slope(), hm.hillshade()])
    for a, b in zip(*runs):
        a, b = _host(a), _host(b)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_dropped_faces_empty_meshes_walls_and_default_grids():
    v = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1], [0, 0, 3], [4, 0, 3], [0, 4, 3], [1, 1, 0], [1, 1, 5], [3, 1, 2], [np.nan, 0, 0], [2, 2, np.inf]], np.float64)
    f = np.array([[3, 4, 5], [0, 1, 2], [6, 7, 8], [0, 1, 99], [0, 1, 9], [0, 2, 1], [-1, 0, 1], [0, 1, 10], [2 ** 40, 0, 1]], np.int64)
    grid = dict(pixel_size=1.0, origin=(0.0, 0.0), shape=(4, 4))
    hm = _rasterizer(v, f).height_map(**grid)
    _same_map('dropped', hm, R.height_map(v, f, **grid))
    assert hm.n_dropped == 5 and hm.n_faces == 9                 # an index past the end, a NaN corner, a negative index, an inf height, 2^40
    assert not bool((hm.layers()[1] == 2).any())                 # the vertical wall covers nothing
    wall = _rasterizer(v, f[2:3]).height_map(**grid)
    assert wall.n_hits == 0 and wall.n_dropped == 0 and wall.n_candidates > 0 and bool((wall.count == 0).all())
    for label, empty in (('no faces', _rasterizer(v, np.zeros((0, 3), np.int32)).height_map(**grid)),
                         ('only dropped faces', _rasterizer(v, f[[3, 4]]).height_map(**grid)),
                         ('a grid off the mesh', _rasterizer(v, f).height_map(1.0, origin=(100.0, -50.0), shape=(4, 4)))):
        assert bool(torch.isnan(empty.height).all()) and bool((empty.face == -1).all()) and bool((empty.count == 0).all()), label
        assert empty.height.shape == (4, 4) and empty.n_hits == 0 and not bool(empty.valid.any()), label
        assert np.array_equal(_host(empty.layers()[0]), np.zeros(17, np.int64)) and empty.layers()[1].shape == (0,), label
        assert bool(torch.isnan(empty.hillshade()).all()) and bool(torch.isnan(empty.sample(np.ones((len(v), 2)))).all()), label
    none = _rasterizer(v, np.zeros((0, 3), np.int32)).height_map(1.0)
    assert none.shape == (0, 0) and none.origin == (0.0, 0.0) and none.height.shape == (0, 0) and _host(none.layers()[0]).tolist() == [0]
    # origin=None and shape=None: every referenced vertex of a valid face lies on the grid
    w, g = _soup(np.float32)
    for p in (0.25, 0.3):
        hm = _rasterizer(w, g).height_map(p)
        ref = R.height_map(w, g, p)
        _same_map('default grid at %g' % p, hm, ref)
        x, y = w[:, 0].astype(np.float64), w[:, 1].astype(np.float64)
        assert hm.origin[0] <= x.min() and hm.origin[1] <= y.min()
        assert x.max() < hm.origin[0] + hm.shape[0] * p and y.max() < hm.origin[1] + hm.shape[1] * p
        assert x.max() >= hm.origin[0] + (hm.shape[0] - 1) * p - 1e-9 and x.min() < hm.origin[0] + p


def test_argument_errors_are_value_errors():
    v, f = _soup(np.float64)
    r = _rasterizer(v, f)
    for bad in (lambda: r.height_map(0.0), lambda: r.height_map(float('nan')), lambda: r.height_map(-1.0), lambda: r.height_map(1e-13),
                lambda: r.height_map(1e-5), lambda: r.height_map(1.0, axes=(0, 0)), lambda: r.height_map(1.0, axes=(0, 3)),
                lambda: r.height_map(1.0, surface='middle'), lambda: r.height_map(1.0, origin=(0.0,)), lambda: r.height_map(1.0, shape=(1 << 16, 1 << 15)),
                lambda: r.height_map(1.0, shape=(4, -1)), lambda: _rasterizer(v, f.astype(np.float32)), lambda: _rasterizer(v[:, :2], f),
                lambda: _rasterizer(v, f, attr=np.zeros((7, 3), np.float32)), lambda: _rasterizer(v, f, attr=np.zeros((len(v), 3), np.int32)),
                lambda: _soup_map(v, f).sample(), lambda: _soup_map(v, f).hillshade(float('inf'))):
        with pytest.raises(ValueError):
            bad()
    assert _soup_map(v, f).n_hits == _soup_ref(np.float64)['n_hits']           # and the rasteriser still works


# ---- derived rasters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 3, 5])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
def test_sample_interpolates_attributes_at_the_hits(dtype, channels):
    v, f = _soup(np.float64)
    ref = _soup_ref(np.float64)
    attr = (np.random.default_rng(channels).normal(size=(len(v), channels)) * 10.0).astype(dtype)
    hm = _rasterizer(v, f, attr).height_map(SOUP['pixel'], SOUP['origin'], SOUP['shape'])
    want = R.sample(v, f, ref, attr)
    got = _host(hm.sample())
    assert got.dtype == np.float64 and got.shape == SOUP['shape'] + (channels,)
    hit = ref['face'] >= 0
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got).all(2), ~hit) and not np.isnan(got[hit]).any()
    bound = 4 * EPS * np.abs(attr.astype(np.float64))[f[ref['face'][hit]]].sum(1)                    # [hits, C]: |t_a| + |t_b| + |t_c|
    err = np.abs(got[hit] - want[hit])
    print('sample %s x %d: largest error %.3g of bound %.3g; bit for bit: %s' % (np.dtype(dtype).name, channels, err.max(), bound.max(),
                                                                                 np.array_equal(got[hit].view(np.int64), want[hit].view(np.int64))))
    assert np.all(err <= bound)
    if channels == 3:                                            # attributes passed to sample() directly, and the coordinates themselves
        assert np.array_equal(_host(_soup_map(v, f).sample(torch.from_numpy(attr))), got, equal_nan=True)
        z = _host(hm.sample(v))[..., 2]
        assert np.array_equal(z[hit].view(np.int64), ref['height'][hit].view(np.int64))              # the height IS the interpolated z


def test_gradient_slope_and_hillshade_on_a_raster_with_holes():
    n, p = 24, 0.5
    gx_, gy_ = np.meshgrid(np.arange(n + 1) * p, np.arange(n + 1) * p, indexing='ij')
    v = np.stack([gx_, gy_, np.sin(0.7 * gx_) * np.cos(0.5 * gy_) + 0.1 * gx_], 2).reshape(-1, 3)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    quads = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], 2).reshape(-1, 4)
    f = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])
    f = f[np.random.default_rng(4).random(len(f)) > 0.03]        # holes
    grid = dict(pixel_size=0.25, origin=(-0.5, -0.5), shape=(53, 52))
    hm = _rasterizer(v, f).height_map(**grid)
    ref = R.height_map(v, f, **grid)
    _same_map('terrain', hm, ref)
    gx, gy = hm.gradient()
    want_x, want_y = R.gradient(ref['height'], 0.25)
    inner = ~np.isnan(want_x)
    holes = np.isnan(want_x[3:-7, 3:-7]).sum()
    print('terrain: %d pixels with a gradient, %d without inside the mesh' % (inner.sum(), holes))
    assert inner.sum() > 1000 and holes > 20 and np.isnan(want_x[0]).all() and np.isnan(want_x[:, -1]).all()
    _same_bits('gx', gx, want_x)
    _same_bits('gy', gy, want_y)
    for azimuth, altitude in ((315.0, 45.0), (135.0, 20.0), (0.0, 90.0)):
        shade = hm.hillshade(azimuth, altitude)
        _same_bits('hillshade %g / %g' % (azimuth, altitude), shade, R.hillshade(ref['height'], 0.25, azimuth, altitude))
        s = _host(shade)[inner]
        assert s.min() >= 0.0 and s.max() <= 1.0 + 2 * EPS
    assert (_host(hm.hillshade(135.0, 20.0))[inner] == 0.0).any()                # somewhere the sun is behind the surface
    slope = _host(hm.slope())
    want = np.arctan(np.hypot(want_x, want_y))
    assert np.array_equal(np.isnan(slope), ~inner)
    err = np.abs(slope[inner] - want[inner]).max()
    print('slope: largest error %.3g of bound %.3g' % (err, 4 * EPS))
    assert err <= 4 * EPS


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def test_meshing_result_height_map():
    import nksr
    from nksr_amd.fields.base_field import MeshingResult
    from nksr_amd.mesh_raster import HeightMap, MeshRasterizer
    assert nksr.MeshRasterizer is MeshRasterizer and nksr.metrics.MeshRasterizer is MeshRasterizer
    v, f = R.snapped_icosphere(1.0, 11.0, 0.0, np.float32)
    colors = np.random.default_rng(9).random((len(v), 3)).astype(np.float32)
    mesh = MeshingResult(torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int32)).cuda(), torch.from_numpy(colors).cuda())
    hm = mesh.height_map(0.5, surface='bottom', axes=(2, 0))
    assert isinstance(hm, HeightMap) and hm.surface == 'bottom' and hm.axes == (2, 0) and hm.up == 1
    ref = R.height_map(v, f, 0.5, surface='bottom', axes=(2, 0))
    _same_map('MeshingResult.height_map', hm, ref)
    direct = MeshRasterizer(v, f, colors).height_map(0.5, surface='bottom', axes=(2, 0))
    assert np.array_equal(_host(hm.sample()), _host(direct.sample()), equal_nan=True) and hm.sample().shape == hm.shape + (3,)
    rgb = _host(hm.sample())[ref['count'] > 0]
    assert rgb.min() >= -4 * EPS and rgb.max() <= 1.0 + 4 * EPS                  # inside the hull of the corner colours
    assert MeshingResult(mesh.v, mesh.f).height_map(0.5).sample(colors).shape[2] == 3


def test_recons_dem_example(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'recons_dem.py'), '0.1', '60000'], cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    print(out.stdout)
    assert 'covered' in out.stdout and 'wrote recons_dem.asc' in out.stdout
    path = str(tmp_path / 'recons_dem.asc')
    with open(path) as fh:
        head = dict(fh.readline().split() for _ in range(6))
    rows = np.loadtxt(path, skiprows=6, ndmin=2)
    assert rows.shape == (int(head['nrows']), int(head['ncols'])) and float(head['cellsize']) == 0.1 and float(head['NODATA_value']) == -9999.0
    covered = rows != -9999.0
    assert rows.size > 1000 and covered.mean() > 0.5 and np.isfinite(rows).all() and np.ptp(rows[covered]) > 0.1
