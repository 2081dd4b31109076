"""numpy references, inputs and check functions for the sparse-network kernels (csrc/nn.hip, the splats of csrc/splat.hip with
splat_for_each_point of csrc/common.h), one kernel at a time.  tests/test_nn_kernels_ref_cpu.py verifies them without a GPU (against
oracle/network.py, against fp32 evaluations in another order, and against deliberately wrong evaluations); tests/test_gpu_nn_kernels.py
hands the kernels' outputs to the same check functions.

Two input families per kernel.

A, lattice.  Inputs whose every product and partial sum is a multiple of one power of two 2^-k and stays below 2^(24 - k): exactly
   representable in fp32 whatever the order of the additions and whether or not a multiply-add is fused.  The comparison is then
   bit for bit and no wrong index can hide behind a tolerance.  Small integers (|v| <= 4) for the dense kernels; for the splats a
   voxel size of 1/8 (inv_w0 = 8 exactly), coordinates on multiples of 1/4 of the finest voxel and small-integer features, which
   makes the per-axis weights multiples of 1/4 at level 0 (1/16 at level 2).  Every lattice reference ASSERTS its own exactness
   condition (`_assert_lattice`): sum |terms| < 2^24 units.  Outputs behind a division or a square root (means, pooling, unit normal,
   sd / sw) are evaluated in fp32 numpy in the kernel's operation order and may differ by 2 ulp (how a compiler rounds a reciprocal
   is not relied on).

B, random fp32.  The reference returns the fp64 value and the fp64 magnitude mag = sum |terms| per output element; the bound is
   |got - ref| <= gamma(m) mag,  gamma(m) = m u / (1 - m u),  u = 2^-24,  m = number of terms + 2 (Higham, Accuracy and Stability of
   Numerical Algorithms, section 3.1: any order of summation, fused or not).  Nothing in it is measured.

A check function takes the "got" arrays and a `report(name, measured, bound)` callable (parity_util.check on the GPU; the default
asserts measured <= bound) and raises AssertionError when a comparison fails.
"""
import numpy as np

from oracle import spec

U = 2.0 ** -24
F32 = np.float32
FAR = np.float32(1e30)
VOXEL = 0.125                       # inv_w0 = 8 exactly
INV_W0 = 8.0
M_CONV, M_LINEAR, M_MLP = 27 * 32 + 2, 32 + 2, 6 + 32 + 4


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def _report(name, measured, bound):
    assert measured <= bound, '%s: measured %.3e > bound %.3e' % (name, measured, bound)


def ulp_distance(a, b):
    """Distance in units of the last place between two finite float32 arrays (0 for +0 against -0)."""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def check_exact(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, '%s: shape %s against %s' % (name, got.shape, ref.shape)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        w = np.argwhere(~same)[0]
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r, expected %r' % (
            name, int((~same).sum()), same.size, tuple(w), got[tuple(w)], ref[tuple(w)]))


def check_ulp(name, got, ref32, ulps=2):
    got, ref32 = np.asarray(got, F32), np.asarray(ref32, F32)
    assert got.shape == ref32.shape, '%s: shape %s against %s' % (name, got.shape, ref32.shape)
    assert np.isfinite(got).all(), '%s: non-finite output' % name
    d = ulp_distance(got, ref32)
    if d.size and d.max() > ulps:
        w = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError('%s: %d ulp at %s: got %r, expected %r' % (name, int(d.max()), w, got[w], ref32[w]))


def bound_ratio(got, ref64, bound):
    """max |got - ref| / bound; an element with bound 0 must match exactly."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape, 'shape %s against %s' % (got.shape, ref64.shape)
    assert np.isfinite(got).all(), 'non-finite output'
    err = np.abs(got - ref64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def _assert_lattice(name, mag, unit_log2):
    """Family A's premise: every partial sum is a multiple of 2^-unit_log2 below 2^24 units, whatever the order."""
    worst = float(np.max(mag)) if np.size(mag) else 0.0
    assert worst * 2.0 ** unit_log2 < 2.0 ** 24, '%s: sum |terms| = %g is not exact on the 2^-%d lattice' % (name, worst, unit_log2)


def _ints(rng, shape, lim=4):
    return rng.integers(-lim, lim + 1, size=shape).astype(F32)


def _values(rng, shape, family, lim=4):
    return _ints(rng, shape, lim) if family == 'A' else rng.standard_normal(shape).astype(F32)


# ---- 3x3x3 sparse convolution ---------------------------------------------------------------------------------------------------------
CONV_N = (1, 31, 32, 33, 127, 128, 129, 257)            # a wavefront owns 32 voxels, a workgroup 128
CONV_KINDS = ('dense', 'holes', 'empty', 'taps25_26')
CONV_MODES = ((True, True), (True, False), (False, True), (False, False))      # (relu, residual)


def conv_nbr(rng, n, kind):
    nbr = rng.integers(0, n, size=(n, 27)).astype(np.int32)
    if kind == 'holes':
        nbr[rng.random((n, 27)) < 0.4] = -1
    elif kind == 'empty':
        nbr[:] = -1
    elif kind == 'taps25_26':
        nbr[:, :25] = -1
    return nbr


def conv_case(n, kind, family, seed=0):
    rng = np.random.default_rng([seed, n, CONV_KINDS.index(kind), int(family == 'A')])
    return dict(n=n, kind=kind, family=family, nbr=conv_nbr(rng, n, kind), x=_values(rng, (n, 32), family), W=_values(rng, (27, 32, 32), family),
                b=_values(rng, 32, family), res=_values(rng, (n, 32), family))


def conv_ref(x, nbr, W, b=None, res=None, relu=False):
    """out[i] = act(b + sum_s W[s]^T x[nbr[i][s]] (+ res[i])) in fp64, and sum |terms| (|b| and |res| included)."""
    n = nbr.shape[0]
    xp = np.concatenate([x.astype(np.float64), np.zeros((1, x.shape[1]))])
    val = np.zeros((n, W.shape[2]))
    mag = np.zeros((n, W.shape[2]))
    for s in range(27):
        val += xp[nbr[:, s]] @ W[s].astype(np.float64)
        mag += np.abs(xp[nbr[:, s]]) @ np.abs(W[s].astype(np.float64))
    if b is not None:
        val, mag = val + b.astype(np.float64), mag + np.abs(b.astype(np.float64))
    if res is not None:
        val, mag = val + res.astype(np.float64), mag + np.abs(res.astype(np.float64))
    return (np.maximum(val, 0.0) if relu else val), mag          # |relu(a) - relu(b)| <= |a - b|: the bound survives the activation


def check_conv(name, case, relu, residual, got_padded, report=_report):
    """``got_padded``: the NaN-filled buffer whose first n rows the kernel was given as `out`."""
    n = case['n']
    got, tail = got_padded[:n], got_padded[n:]
    assert tail.size and np.isnan(tail).all(), '%s: a row behind n was written' % name
    val, mag = conv_ref(case['x'], case['nbr'], case['W'], case['b'], case['res'] if residual else None, relu)
    if case['family'] == 'A':
        _assert_lattice(name, mag, 0)
        check_exact(name, got, val.astype(F32))
    else:
        report(name, bound_ratio(got, val, gamma(M_CONV) * mag), 1.0)


def conv_dgrad_ref(gz, nbr, W):
    """The fp64 transpose of conv_ref: gin[nbr[i][s]] += W[s] gz[i]."""
    n = nbr.shape[0]
    val, mag = np.zeros((n + 1, 32)), np.zeros((n + 1, 32))
    g = gz.astype(np.float64)
    for s in range(27):
        np.add.at(val, nbr[:, s], g @ W[s].astype(np.float64).T)
        np.add.at(mag, nbr[:, s], np.abs(g) @ np.abs(W[s].astype(np.float64)).T)
    return val[:n], mag[:n]


def check_dgrad(name, family, gz, nbr, W, got, report=_report):
    val, mag = conv_dgrad_ref(gz, nbr, W)
    if family == 'A':
        _assert_lattice(name, mag, 0)
        check_exact(name, got, val.astype(F32))
    else:
        report(name, bound_ratio(got, val, gamma(M_CONV) * mag), 1.0)


def nbr_symmetric(nbr):
    """nbr[nbr[i][s]][26 - s] == i wherever nbr[i][s] >= 0: what the mirrored-tap data gradient rests on."""
    i = np.arange(nbr.shape[0])[:, None]
    s = np.arange(27)[None]
    j = nbr
    back = nbr[np.maximum(j, 0), 26 - s]
    return bool(((j < 0) | (back == i)).all())


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
WGRAD_N = (1, 2, 7, 8, 9, 2047, 2048, 2049)             # chunks of 2048, 8 voxels per trip, pairs of voxels per instruction
WGRAD_CHUNK = 2048


def wgrad_case(n, family, seed=1):
    rng = np.random.default_rng([seed, n, int(family == 'A')])
    return dict(n=n, family=family, nbr=conv_nbr(rng, n, 'holes'), x=_values(rng, (n, 32), family), gz=_values(rng, (n, 32), family))


def wgrad_ref(x, nbr, gz):
    xp = np.concatenate([x.astype(np.float64), np.zeros((1, 32))])
    g = gz.astype(np.float64)
    val = np.stack([xp[nbr[:, s]].T @ g for s in range(27)])
    mag = np.stack([np.abs(xp[nbr[:, s]]).T @ np.abs(g) for s in range(27)])
    return val, mag


def check_wgrad(name, case, got, report=_report):
    val, mag = wgrad_ref(case['x'], case['nbr'], case['gz'])
    if case['family'] == 'A':
        _assert_lattice(name, mag, 0)
        check_exact(name, got, val.astype(F32))
    else:
        report(name, bound_ratio(got, val, gamma(case['n'] + 2) * mag), 1.0)


# ---- linear head ------------------------------------------------------------------------------------------------------------------
LINEAR_CASES = ((1, 7), (3, 87), (4, 65), (32, 9), (32, 1), (3, 1))      # (Cout, n): n * Cout is never a multiple of 256


def linear_case(cout, n, family, seed=2):
    rng = np.random.default_rng([seed, cout, n, int(family == 'A')])
    return dict(n=n, cout=cout, family=family, x=_values(rng, (n, 32), family), W=_values(rng, (cout, 32), family), b=_values(rng, cout, family))


def linear_ref(x, W, b=None):
    val = x.astype(np.float64) @ W.astype(np.float64).T
    mag = np.abs(x.astype(np.float64)) @ np.abs(W.astype(np.float64)).T
    if b is not None:
        val, mag = val + b.astype(np.float64), mag + np.abs(b.astype(np.float64))
    return val, mag


def check_linear(name, case, with_bias, got, report=_report):
    val, mag = linear_ref(case['x'], case['W'], case['b'] if with_bias else None)
    if case['family'] == 'A':
        _assert_lattice(name, mag, 0)
        check_exact(name, got, val.astype(F32))
    else:
        report(name, bound_ratio(got, val, gamma(M_LINEAR) * mag), 1.0)


# ---- point MLP --------------------------------------------------------------------------------------------------------------------
MLP_N = (1, 63, 64, 65, 255, 256, 257)                  # a wavefront writes a 64-row image; the last one may be partial


def mlp_case(n, family, seed=3):
    rng = np.random.default_rng([seed, n, int(family == 'A')])
    if family == 'A':
        xyz = (rng.integers(-40, 40, size=(n, 3)).astype(F32) / F32(32.0)).astype(F32)      # multiples of 1/4 voxel, negative cells included
    else:
        xyz = rng.uniform(-1.2, 1.2, size=(n, 3)).astype(F32)
    if n > 1:
        xyz[0] = -np.abs(xyz[0]) - F32(0.125)                                                # (a point in a negative cell on every axis)
    return dict(n=n, family=family, xyz=xyz, feat=_values(rng, (n, 3), family), W1=_values(rng, (32, 6), family), b1=_values(rng, 32, family),
                W2=_values(rng, (32, 32), family), b2=_values(rng, 32, family))


def mlp_input(xyz, feat, inv_w0=INV_W0):
    """[u - 1/2, feat] as the kernel forms it: p = fl(x inv_w0), I = floor(fl(2 p)) >> 1, (p - I) - 1/2 in fp32 (IEEE operations,
    nothing fused: the same bits in numpy)."""
    p = (xyz.astype(F32) * F32(inv_w0)).astype(F32)
    cell = np.floor(p * F32(2.0)).astype(np.int32) >> 1
    u = ((p - cell.astype(F32)).astype(F32) - F32(0.5)).astype(F32)
    return np.concatenate([u, feat.astype(F32)], 1)


def mlp_ref(case):
    """fp64 value and magnitude from the fp32 input row.  The first layer's error (8 roundings on |b1| + |W1||in|) is carried through
    |W2| into the second one's (34): m = 6 + 32 + 4 on mag = |b2| + |W2| (|b1| + |W1| |in|)."""
    x = mlp_input(case['xyz'], case['feat']).astype(np.float64)
    W1, b1, W2, b2 = (case[k].astype(np.float64) for k in ('W1', 'b1', 'W2', 'b2'))
    h = np.maximum(x @ W1.T + b1, 0.0)
    hm = np.abs(x) @ np.abs(W1).T + np.abs(b1)
    return h @ W2.T + b2, hm @ np.abs(W2).T + np.abs(b2)


def check_mlp(name, case, got_padded, report=_report):
    n = case['n']
    got, tail = got_padded[:n], got_padded[n:]
    assert tail.size and np.isnan(tail).all(), '%s: a row behind n was written' % name
    val, mag = mlp_ref(case)
    if case['family'] == 'A':
        assert (np.abs(mlp_input(case['xyz'], case['feat'])[:, :3] * 4) % 1 == 0).all()
        _assert_lattice(name, mag, 2)
        check_exact(name, got, val.astype(F32))
    else:
        report(name, bound_ratio(got, val, gamma(M_MLP) * mag), 1.0)


# ---- pooling, gathers ----------------------------------------------------------------------------------------------------------------
def pool_case(n_parent, C, seed=4):
    """Children ranges of 0, 1 and 8 (and, with 9 parents, other sizes) over a contiguous child array."""
    rng = np.random.default_rng([seed, n_parent, C])
    sizes = np.array([8] if n_parent == 1 else [8, 0, 1, 3, 8, 0, 5, 1, 2][:n_parent])
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    end = (start + sizes).astype(np.int32)
    return dict(n_parent=n_parent, C=C, start=start, end=end, child=_ints(rng, (int(sizes.sum()), C)))


def pool_ref32(case):
    out = np.zeros((case['n_parent'], case['C']), F32)
    for p, (k0, k1) in enumerate(zip(case['start'], case['end'])):
        if k1 > k0:
            a = case['child'][k0:k1].astype(np.float64).sum(0).astype(F32)        # (integers: exact)
            out[p] = a / F32(k1 - k0)
    return out


def check_pool(name, case, got):
    sizes = case['end'] - case['start']
    assert {0, 1, 8} <= set(sizes.tolist()) or case['n_parent'] == 1
    check_exact(name + ':empty ranges', got[sizes == 0], np.zeros((int((sizes == 0).sum()), case['C']), F32))
    check_ulp(name, got, pool_ref32(case), 2)


# ---- trilinear splats -------------------------------------------------------------------------------------------------------------
def crafted_cells():
    """(level-0 cell, number of points) of the crafted cloud: see `cloud_edges` for what it must contain."""
    cells = [((0, 0, 0), 320),                       # many rounds of the 4-per-lane list; > 128 list entries at the voxels around it
             ((1, 0, 0), 40), ((0, 1, 1), 33),
             ((-3, -2, -4), 4), ((-3, -2, -3), 5),    # the round boundary, at negative coordinates
             ((9, 9, 9), 1),                         # an isolated single point
             ((-9, 6, 2), 1), ((-8, 7, 3), 1)]       # two points in diagonal cells: 15 voxels (an odd count)
    k = 0
    for x in range(4, 9):                            # a compact block of 1..25-point cells (some empty), negative y
        for y in range(-6, -1):
            for z in range(10, 14):
                k += 1
                if k % 11:
                    cells.append(((x, y, z), 1 + (k * 7) % 25))
    return cells


def crafted_cloud(family, seed=5):
    """About 1500 points, given by their level-0 cell and a position inside it: a multiple of 1/4 voxel (family A), or that plus a
    random fp32 offset below 1/4 (B).  Returns (xyz, normal), unsorted."""
    rng = np.random.default_rng(seed)
    cell = np.concatenate([np.tile(np.array(c, np.int64), (k, 1)) for c, k in crafted_cells()])
    frac = rng.integers(0, 4, size=cell.shape).astype(np.float64) / 4.0
    lone = np.array([c for c, k in crafted_cells() if k == 1][:3], np.int64)
    for c in lone:                                   # the hand-placed single points sit at 1/4: their footprint is known
        frac[(cell == c).all(1)] = 0.25
    if family != 'A':                                # the same half cells (hence the same grids at every level), any fp32 inside them
        frac = frac + rng.uniform(0.02, 0.23, size=cell.shape)
    xyz = ((cell + frac) * VOXEL).astype(F32)
    normal = _values(rng, cell.shape, family, lim=2)
    perm = rng.permutation(len(xyz))                 # unsorted, as a cloud arrives
    return xyz[perm], normal[perm]


def cloud_cells(xyz, level=0):
    h0, _ = spec.half_index(xyz, VOXEL)
    return (h0 >> level) >> 1


def splat_weights(xyz, ijk, inv_w):
    """Dense gather over ALL points: fp32 trilinear weights [n_voxel, n_point] as the kernels form them (w = (wx wy) wz of
    w_a = 1 - |fl(x inv_w) - centre|, zero unless every w_a > 0), the offsets r [n_voxel, n_point, 3] and the number of points that
    lie exactly on a weight-0 plane of a voxel whose stencil holds them."""
    p = (xyz.astype(F32) * F32(inv_w)).astype(F32)
    c = ijk.astype(F32) + F32(0.5)
    r = (p[None, :, :] - c[:, None, :]).astype(F32)
    wa = (F32(1.0) - np.abs(r)).astype(F32)
    keep = (wa > 0).all(2)
    w = ((wa[..., 0] * wa[..., 1]).astype(F32) * wa[..., 2]).astype(F32)
    on_plane = int(((wa >= 0).all(2) & (wa == 0).any(2)).sum())
    return np.where(keep, w, F32(0)), r, keep, on_plane


class SplatRef:
    """Everything the splat checks need for one (cloud, level grid): computed once, shared by the sum / mean / plane checks."""

    def __init__(self, xyz_sorted, ijk, level, family):
        self.family, self.level = family, level
        self.inv_w = INV_W0 * 2.0 ** (-level)
        self.unit = 6 if level == 0 else 12          # weights are multiples of 2^-6 (per axis 1/4) at level 0, 2^-12 (1/16) at level 2
        self.xyz, self.ijk = xyz_sorted, ijk
        self.w32, self.r32, self.keep, self.on_plane = splat_weights(xyz_sorted, ijk, self.inv_w)
        self.w = self.w32.astype(np.float64)
        self.cnt = self.keep.sum(1)
        self.wsum = self.w.sum(1)
        if family == 'A':
            assert level in (0, 2)
            _assert_lattice('weight sum', self.wsum, self.unit)

    def sums(self, feat):
        f = feat.astype(np.float64)
        return self.w @ f, self.w @ np.abs(f)

    def check_sum(self, name, feat, got, got_ws, report=_report):
        """k_splat_trilinear: fp64 accumulators, one rounding to fp32 at the end (2 u mag: the fp64 roundings are 2^-29 of that)."""
        val, mag = self.sums(feat)
        if self.family == 'A':
            _assert_lattice(name, mag, self.unit)
            check_exact(name + ':sum', got, val.astype(F32))
            check_exact(name + ':wsum', got_ws, self.wsum.astype(F32))
        else:
            report(name + ':sum', bound_ratio(got, val, 2 * U * mag), 1.0)
            report(name + ':wsum', bound_ratio(got_ws, self.wsum, 2 * U * self.wsum), 1.0)
        empty = self.cnt == 0
        check_exact(name + ':untouched voxels', np.asarray(got)[empty], np.zeros((int(empty.sum()), feat.shape[1]), F32))

    def check_mean(self, name, feat, got, report=_report):
        val, mag = self.sums(feat)
        occ = self.cnt > 0
        check_exact(name + ':untouched voxels', np.asarray(got)[~occ], np.zeros((int((~occ).sum()), feat.shape[1]), F32))
        if self.family == 'A':
            _assert_lattice(name, mag, self.unit)
            inv = np.where(occ, F32(1.0) / np.where(occ, self.wsum, 1.0).astype(F32), F32(0)).astype(F32)
            check_ulp(name, got, (val.astype(F32) * inv[:, None]).astype(F32), 2)
        else:
            ws = np.where(occ, self.wsum, 1.0)[:, None]
            report(name, bound_ratio(got, val / ws, gamma(2 * self.cnt + 4)[:, None] * mag / ws), 1.0)

    def check_plane(self, name, normal, got, report=_report):
        """out [n, 8] = (occupied, sum w r / sum w, unit sum w n, 0)."""
        got = np.asarray(got)
        occ = self.cnt > 0
        check_exact(name + ':occupied', got[:, 0], occ.astype(F32))
        check_exact(name + ':pad', got[:, 7], np.zeros(len(occ), F32))
        check_exact(name + ':untouched voxels', got[~occ], np.zeros((int((~occ).sum()), 8), F32))
        r = self.r32.astype(np.float64)
        osum = np.einsum('vp,vpa->va', self.w, r)
        omag = np.einsum('vp,vpa->va', self.w, np.abs(r))
        nsum, nmag = self.sums(normal)
        if self.family == 'A':
            _assert_lattice(name + ':offset', omag, self.unit + (2 if self.level == 0 else 4))
            _assert_lattice(name + ':normal', nmag, self.unit)
            inv = np.where(occ, F32(1.0) / np.where(occ, self.wsum, 1.0).astype(F32), F32(0)).astype(F32)
            check_ulp(name + ':offset', got[:, 1:4], (osum.astype(F32) * inv[:, None]).astype(F32), 2)
            n32 = nsum.astype(F32)
            nn = np.sqrt(((n32[:, 0] * n32[:, 0] + n32[:, 1] * n32[:, 1]).astype(F32) + n32[:, 2] * n32[:, 2]).astype(F32)).astype(F32)
            big = nn > F32(1e-8)
            invn = np.where(big, F32(1.0) / np.where(big, nn, F32(1)), F32(0)).astype(F32)
            check_ulp(name + ':normal', got[:, 4:7], (n32 * invn[:, None]).astype(F32), 2)
        else:
            ws = np.where(occ, self.wsum, 1.0)[:, None]
            report(name + ':offset', bound_ratio(got[:, 1:4], osum / ws, gamma(2 * self.cnt + 4)[:, None] * omag / ws), 1.0)
            # the one amplified output: d(N / |N|) = (I - u u^T) dN / |N|, so every component moves by at most |dN|_2 / |N|; the
            # normalisation's own six roundings are relative to |u_c| <= 1 <= |mag|_2 / |N| and join m
            nl = np.linalg.norm(nsum, axis=1)
            assert (nl[occ] > 1e-6).all()
            unit = nsum / np.where(occ, nl, 1.0)[:, None]
            bnd = gamma(self.cnt + 8) * np.linalg.norm(nmag, axis=1) / np.where(occ, nl, 1.0)
            report(name + ':normal', bound_ratio(got[:, 4:7], unit * occ[:, None], np.where(occ, bnd, 0.0)[:, None] * np.ones((1, 3))), 1.0)


def site_ranges_ref(site_keys, vox_keys, level):
    return (np.searchsorted(site_keys, vox_keys << (3 * level)).astype(np.int32),
            np.searchsorted(site_keys, (vox_keys + 1) << (3 * level)).astype(np.int32))


def cloud_edges(xyz, grid_ijk0, cnt0):
    """What the crafted cloud must contain (level-0 splatting grid ``grid_ijk0``, per-voxel list lengths ``cnt0``)."""
    cell = cloud_cells(xyz)
    uc, per = np.unique(cell, axis=0, return_counts=True)
    have = set(map(tuple, uc.tolist()))
    lonely = [c for c, k in zip(uc.tolist(), per) if k == 1 and not any(
        (c[0] + o[0], c[1] + o[1], c[2] + o[2]) in have for o in spec.NBR_OFFSETS.tolist() if any(o))]
    p = xyz.astype(F32) * F32(INV_W0)
    return dict(points=len(xyz), big_cell=int(per.max()), cell_of_4=bool((per == 4).any()), cell_of_5=bool((per == 5).any()),
                longest_list=int(cnt0.max()), on_centre=int(((p - np.floor(p)) == 0.5).any(1).sum()), negative=bool((xyz < 0).all(1).any()),
                isolated=len(lonely), voxels=len(grid_ijk0))


def assert_cloud_edges(e, family):
    assert 1300 <= e['points'] <= 1800, e
    assert e['big_cell'] >= 300 and e['cell_of_4'] and e['cell_of_5'] and e['longest_list'] > 128, e
    assert e['negative'] and e['isolated'] >= 1 and e['voxels'] % 2 == 1, e
    if family == 'A':
        assert e['on_centre'] >= 100, e            # a coordinate on a cell centre: weight exactly 0 at the voxels one step away


# ---- UDF decode --------------------------------------------------------------------------------------------------------------------
def udf_case(seed=6):
    """One level: a 5 x 4 x 4 block of voxels with holes (hash misses), plane features on the lattice with occupied and unoccupied
    voxels, and queries on multiples of 1/4 voxel in and around it."""
    rng = np.random.default_rng(seed)
    ijk = np.array([[x, y, z] for x in range(-3, 2) for y in range(-2, 2) for z in range(0, 4)], np.int32)
    ijk = ijk[(rng.random(len(ijk)) > 0.2) | (ijk[:, 0] >= 0)]
    feat = np.zeros((len(ijk), 8), F32)
    feat[:, 0] = (rng.random(len(ijk)) > 0.35) | (ijk[:, 0] >= 0)            # x >= 0: every present voxel is occupied
    feat[:, 1:4] = rng.integers(-2, 3, size=(len(ijk), 3)) / 4.0
    feat[:, 4:7] = rng.integers(-2, 3, size=(len(ijk), 3))
    q = rng.integers(-18, 14, size=(400, 3)).astype(F32) / F32(4.0)
    q[:, 2] += F32(1.0)
    q[:40] = rng.integers(2, 6, size=(40, 3)).astype(F32) / F32(4.0) + np.array([0, -1, 1], F32)
    return dict(ijk=ijk, feat=feat, xyz=(q * F32(VOXEL)).astype(F32), level=0)


def udf_ref32(ijk, feat, xyz, inv_w, w, only_unset=False, prev=None, stats=None):
    """k_udf_decode in fp32 numpy, its operation order (on the lattice d, t and the sums are exact; sd / sw is the one rounding)."""
    table = {tuple(c): j for j, c in enumerate(ijk.tolist())}
    p = (xyz.astype(F32) * F32(inv_w)).astype(F32)
    fl = np.floor(p - F32(0.5))
    base = fl.astype(np.int64)
    v = (p - F32(0.5) - fl).astype(F32)
    out = np.full(len(xyz), FAR, F32) if prev is None else prev.copy()
    st = dict(all8=0, some=0, none=0, unoccupied_corners=0, absent_corners=0)
    for i in range(len(xyz)):
        if only_unset and out[i] < F32(0.5) * FAR:
            continue
        sw, sd, hit = F32(0), F32(0), 0
        for co in spec.CORNER_OFFSETS:
            j = table.get(tuple((base[i] + co).tolist()), -1)
            if j < 0:
                st['absent_corners'] += 1
                continue
            f = feat[j]
            if not f[0] > F32(0.5):
                st['unoccupied_corners'] += 1
                continue
            t = F32(1)
            for a in range(3):
                t = F32(t * (v[i, a] if co[a] else F32(1) - v[i, a]))
            rr = [F32(F32(p[i, a] - (F32(base[i, a] + co[a]) + F32(0.5))) - f[1 + a]) for a in range(3)]
            d = F32(rr[0] * f[4] + F32(rr[1] * f[5] + F32(rr[2] * f[6])))
            sw, sd, hit = F32(sw + t), F32(sd + F32(t * d)), hit + 1
        st['all8' if hit == 8 else 'some' if hit else 'none'] += 1
        if sw > 0:
            out[i] = F32(np.abs(F32(sd / sw)) * F32(w))
        elif not only_unset:
            out[i] = FAR
    if stats is not None:
        stats.update(st)
    return out


def udf_prev(case, fresh, seed=7):
    """The state a finer level leaves behind: about half of the decodable entries hold a value (not this level's), the rest 1e30."""
    rng = np.random.default_rng(seed)
    marker = (F32(0.015625) * (1 + np.arange(len(fresh)) % 5)).astype(F32)
    return np.where((rng.random(len(fresh)) < 0.5) & (fresh < F32(0.5) * FAR), marker, FAR).astype(F32)


def check_udf(name, ref32, got):
    got = np.asarray(got, F32)
    far = ref32 >= F32(0.5) * FAR
    check_exact(name + ':FAR', got[far], ref32[far])
    check_ulp(name, got[~far], ref32[~far], 2)


def check_udf_only_unset(name, case, prev, got, inv_w=INV_W0, w=VOXEL):
    """A second pass with only_unset = 1 over ``prev``: decoded entries stay bit-identical, entries at 1e30 are (still) filled."""
    got = np.asarray(got, F32)
    done = prev < F32(0.5) * FAR
    assert done.any() and (~done).any()
    check_exact(name + ':kept', got[done], prev[done])
    fresh = udf_ref32(case['ijk'], case['feat'], case['xyz'], inv_w, w)
    assert (fresh[~done] < F32(0.5) * FAR).any(), '%s: no unset entry can be filled' % name
    check_udf(name + ':filled', fresh[~done], got[~done])
