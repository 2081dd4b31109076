"""The kernel field by its definition, in fp64, for the four device routines that evaluate it (csrc/kfield.hip: k_voxel_psi,
k_kernel_rows, k_kernel_factors; csrc/evalf.hip: k_evaluate_f, k_evaluate_f_grad), with the cases they are held to.
tests/test_kernel_field_ref_cpu.py verifies the reference and the cases without a GPU (the fp32 oracle meets the bound, mutations of
the oracle miss it); tests/test_gpu_kernel_field.py hands the kernels' outputs to the same comparison.

    K_d(x, c_j) = <phi_d(x), psi_j> B((x - c_j) / w_d),     f(x) = sum_d sum_j alpha_j K_d(x, c_j)

The reference knows no cells, no slots and no neighbour tables: every sum runs over ALL voxels of a level, and a voxel that does not
exist contributes nothing because it is not in the sum.

The one fp32 step taken as given is  p = fp32(x) * fp32(1 / voxel_size)  (oracle/spec.py: half_index).  From p on everything is
exact in fp64:  q_d = p 2^-d,  r = q_d - (ijk + 0.5)  per voxel (both exact: p has 24 bits).
  trilinear features   t = sum_j feat_j prod_a hat(r_a),  hat(r) = max(0, 1 - |r|)
  tangents             Jt_a = inv_w_d sum_j feat_j hat'(r_a) prod_{b != a} hat(r_b)  with the RIGHT derivative of hat: +1 on [-1, 0),
                       -1 on [0, 1), 0 elsewhere -- what the kernels' half-open cells and half cells mean
  interpolator         phi = t + W3 relu(W2 relu(W1 t + b1) + b2) + b3,  J = its forward-mode tangent with the masks of the fp64
                       pre-activations,  psi_j = phi(feat_j)
  spline               B(r) = prod_a b(r_a),  b(r) = 0.75 - r^2 (|r| < 0.5), 0.5 (1.5 - |r|)^2 (0.5 <= |r| < 1.5), support [-1.5, 1.5),
                       and b'(r) in the same closed form.

The bound is derived, not measured:  |got - ref| <= gamma(m) mag,  gamma(m) = m u / (1 - m u),  u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: any order of summation, fused or not).

mag is the same chain evaluated with absolute values throughout (|feat|, |W|, |b|, |alpha|, |J| terms): the sum of |terms| that a
running error bound multiplies.  ReLU is 1-Lipschitz, so a layer's error passes through it undiminished at worst and mag(relu(a)) =
mag(a): values, rows and phi need no exclusion.  One thing in the chain has an ABSOLUTE error, not a relative one: the local
coordinate.  u = p 2^-d - I rounds when p < 0, v = u + 0.5 - hb rounds once more, and a 1-D weight formed from them (1 - v, 0.5 (1 -
u)^2, ...) can be 2^-25 with an error of 2^-25.  Every 1-D weight and 1-D spline derivative is within ABS_W u of its exact value
(slopes <= 2, two roundings of size u / 2, one of the weight's own), so mag evaluates them as |w| + TAU on their support with gamma(m)
TAU = ABS_W u:  gamma(m) prod_a (|w_a| + TAU) covers gamma(m) prod |w_a| and the first-order absolute terms at once.

m, the number of roundings on the longest chain of one output (chain_length):
     11   trilinear stencil: two products for the corner weight, eight fused multiply-adds, the factor inv_w of a tangent
  2 (K + 2 H + 4)   the interpolator, layer by layer (K + 1, H + 1, H + 2), once for phi(x) and once for psi_j: both come from fp32
      K   the dot product <phi, psi_j>
     16   spline: three roundings per 1-D weight (9), B (2), the derivative factor and inv_w (3), dot * B, the J term's multiply-add
     27   the slots of a level, one multiply-add each
  depth   the level sum
      5   alpha * psi of the pre-multiplied path, row_scale, and three to spare
The Jacobian J is discontinuous where a pre-activation crosses 0, so what uses J (exact gradients, the J records of the factor form)
is compared only at queries whose ReLU margin -- the minimum over the touched levels and all hidden units of |pre-activation| /
mag(pre-activation) -- exceeds 2 gamma(m): there the fp32 masks are the fp64 masks.  At most MAX_EXCLUDED of a case's queries may fall
to this (asserted on the CPU).
"""
import functools

import numpy as np

from nn_kernels_ref import U, bound_ratio, gamma        # noqa: F401  (re-exported: one gamma for every reference module)
from oracle import spec

F32 = np.float32
F64 = np.float64
VOXEL = 0.1                 # parity_util.field_inputs builds every hierarchy at this voxel size
MAX_DEPTH = 6               # NKSR_MAX_DEPTH (include/nksr_hip.h)
ABS_W = 3.0                 # absolute error of a 1-D weight, in units of u
MAX_EXCLUDED = 0.05         # share of a case's queries that the ReLU margin may exclude from the exact-gradient checks


def psi_chain(K, H):
    """roundings of one interpolator evaluation (psi alone: nksr_voxel_psi)"""
    return K + 2 * H + 4


def chain_length(K, H, depth):
    return 11 + 2 * psi_chain(K, H) + K + 16 + 27 + depth + 5


class RefLevel:
    """One level's inputs in fp64: integer coordinates [n, 3], features [n, K], the six interpolator arrays, alpha [n]."""

    def __init__(self, ijk, feat, W1, b1, W2, b2, W3, b3, alpha):
        self.ijk = np.asarray(ijk, np.int64)
        self.feat, self.alpha = np.asarray(feat, F64), np.asarray(alpha, F64)
        self.W1, self.b1, self.W2, self.b2, self.W3, self.b3 = [np.asarray(a, F64) for a in (W1, b1, W2, b2, W3, b3)]
        self.n = self.ijk.shape[0]


def interpolator(lv, t, mt, Jt=None, mJt=None):
    """phi, mag(phi), the ReLU margin per row, the ReLU masks [n, 2 H] and (with tangents [n, K, 3]) J, mag(J)."""
    aW1, aW2, aW3 = np.abs(lv.W1), np.abs(lv.W2), np.abs(lv.W3)
    a1 = t @ lv.W1.T + lv.b1
    m1 = mt @ aW1.T + np.abs(lv.b1)
    a2 = np.maximum(a1, 0) @ lv.W2.T + lv.b2
    m2 = m1 @ aW2.T + np.abs(lv.b2)
    phi = t + np.maximum(a2, 0) @ lv.W3.T + lv.b3
    mphi = mt + m2 @ aW3.T + np.abs(lv.b3)
    with np.errstate(divide='ignore', invalid='ignore'):         # (mag 0: the pre-activation is 0 on both sides, the unit is off)
        rel = np.concatenate([np.where(m1 > 0, np.abs(a1) / m1, np.inf), np.where(m2 > 0, np.abs(a2) / m2, np.inf)], 1)
    margin, masks = rel.min(1), np.concatenate([a1 > 0, a2 > 0], 1)
    if Jt is None:
        return phi, mphi, margin, masks, None, None
    d1 = np.einsum('hk,nka->nha', lv.W1, Jt) * (a1 > 0)[:, :, None]
    d2 = np.einsum('gh,nha->nga', lv.W2, d1) * (a2 > 0)[:, :, None]
    J = Jt + np.einsum('kg,nga->nka', lv.W3, d2)
    mJ = mJt + np.einsum('kj,nja->nka', aW3 @ aW2 @ aW1, mJt)
    return phi, mphi, margin, masks, J, mJ


def voxel_psi(lv):
    """psi_j = phi(feat_j) and its mag."""
    psi, mpsi = interpolator(lv, lv.feat, np.abs(lv.feat))[:2]
    return psi, mpsi


def _hat(r, tau):
    sup = (r >= -1.0) & (r < 1.0)
    w = np.where(sup, 1.0 - np.abs(r), 0.0)
    dw = np.where(sup, np.where(r < 0.0, 1.0, -1.0), 0.0)        # the right derivative
    return w, dw, np.where(sup, w + tau, 0.0), sup.astype(F64)   # (the derivative is +-1 exactly: its mag is 1)


def _spline(r, tau):
    ar = np.abs(r)
    sup = (r >= -1.5) & (r < 1.5)
    inner = ar < 0.5
    w = np.where(inner, 0.75 - r * r, np.where(sup, 0.5 * (1.5 - ar) ** 2, 0.0))
    dw = np.where(inner, -2.0 * r, np.where(sup, -(1.5 - ar) * np.sign(r), 0.0))
    return w, dw, np.where(sup, w + tau, 0.0), np.where(sup, np.abs(dw) + tau, 0.0)


def _prod3(x, y, z):
    return x[..., 0] * y[..., 1] * z[..., 2]


class FieldRef:
    """The field of ``levels`` (RefLevel, fine -> coarse) at the queries ``xyz`` [n, 3] fp32.  Per level d the lists hold
    phi / mphi [n, K], J / mJ [n, K, 3] (world units), margin [n], active [n] (floor(q_d) is a voxel), cell [n] (its index or -1),
    and over ALL voxels of the level the kernel values Kv [n, n_d] and derivatives dKa (approx) / dKe (exact) [n, 3, n_d], each with
    its mag (m-prefixed)."""

    def __init__(self, levels, xyz, voxel_size=VOXEL, p32=None):
        self.levels = levels
        self.depth = len(levels)
        K, H = levels[0].feat.shape[1], levels[0].W1.shape[0]
        self.K, self.H = K, H
        self.m = chain_length(K, H, self.depth)
        self.g = float(gamma(self.m))
        tau = ABS_W * U / self.g
        inv_w0 = spec.inv_w0_f32(voxel_size)
        # the one fp32 step (``p32``: the products themselves, for the tests of this reference)
        self.p32 = (np.asarray(xyz, F32) * inv_w0).astype(F32) if p32 is None else np.asarray(p32, F32)
        p = self.p32.astype(F64)
        n = p.shape[0]
        self.n = n
        self.offsets = np.concatenate([[0], np.cumsum([lv.n for lv in levels])]).astype(np.int64)
        self.lv = []
        for d, lv in enumerate(levels):
            q = p * 2.0 ** -d
            inv_w = float(inv_w0) * 2.0 ** -d
            cellijk = np.floor(q).astype(np.int64)
            r = q[:, None, :] - (lv.ijk[None].astype(F64) + 0.5)                       # [n, n_d, 3]
            D = lv.ijk[None] - cellijk[:, None]                                        # voxel - containing cell
            inslot = (np.abs(D) <= 1).all(-1)
            home = (D == 0).all(-1)
            active = home.any(1)
            cell = np.where(active, home.argmax(1), -1)
            hw, hd, hwm, hdm = _hat(r, tau)
            af = np.abs(lv.feat)
            t, mt = _prod3(hw, hw, hw) @ lv.feat, _prod3(hwm, hwm, hwm) @ af
            Jt = np.stack([_prod3(hd, hw, hw) @ lv.feat, _prod3(hw, hd, hw) @ lv.feat, _prod3(hw, hw, hd) @ lv.feat], -1) * inv_w
            mJt = np.stack([_prod3(hdm, hwm, hwm) @ af, _prod3(hwm, hdm, hwm) @ af, _prod3(hwm, hwm, hdm) @ af], -1) * inv_w
            phi, mphi, margin, masks, J, mJ = interpolator(lv, t, mt, Jt, mJt)
            psi, mpsi = voxel_psi(lv)
            bw, bd, bwm, bdm = _spline(r, tau)
            B, mB = _prod3(bw, bw, bw), _prod3(bwm, bwm, bwm)
            dB = np.stack([_prod3(bd, bw, bw), _prod3(bw, bd, bw), _prod3(bw, bw, bd)], 1) * inv_w      # [n, 3, n_d]
            mdB = np.stack([_prod3(bdm, bwm, bwm), _prod3(bwm, bdm, bwm), _prod3(bwm, bwm, bdm)], 1) * inv_w
            dot, mdot = phi @ psi.T, mphi @ mpsi.T
            jd = np.einsum('nka,jk->naj', J, psi)
            mjd = np.einsum('nka,jk->naj', mJ, mpsi)
            dKa, mdKa = dot[:, None] * dB, mdot[:, None] * mdB
            self.lv.append(dict(
                phi=phi, mphi=mphi, J=J, mJ=mJ, t=t, margin=margin, masks=masks,
                active=active, cell=cell, inslot=inslot, D=D, touched=inslot.any(1),
                psi=psi, mpsi=mpsi, Kv=dot * B, mKv=mdot * mB, dKa=dKa, mdKa=mdKa, dKe=dKa + jd * B[:, None], mdKe=mdKa + mjd * mB[:, None]))

    # ---- f and its gradients --------------------------------------------------------------------------------------------------
    def _sum(self, key, alpha, active_only):
        out = mag = 0.0
        for d, (lv, R) in enumerate(zip(self.levels, self.lv)):
            a = lv.alpha if alpha is None else np.asarray(alpha, F64)[self.offsets[d]:self.offsets[d + 1]]
            keep = R['active'] if active_only else np.ones(self.n, bool)
            keep = keep.reshape((-1,) + (1,) * (R[key].ndim - 2))
            out = out + np.where(keep, R[key] @ a, 0.0)
            mag = mag + np.where(keep, R['m' + key] @ np.abs(a), 0.0)
        return out, mag

    def value(self, alpha=None, active_only=False):
        """f [n] and its mag."""
        return self._sum('Kv', alpha, active_only)

    def gradient(self, exact, alpha=None, active_only=False):
        """grad f [n, 3] (exact: with the J term; else the approximate gradient that drops it) and its mag."""
        return self._sum('dKe' if exact else 'dKa', alpha, active_only)

    def margin(self, active_only=False):
        """Per query: min over the touched levels (a slot voxel exists; active_only: the containing cell does) of the ReLU margin."""
        out = np.full(self.n, np.inf)
        for R in self.lv:
            use = R['active'] if active_only else R['touched']
            out = np.minimum(out, np.where(use, R['margin'], np.inf))
        return out

    def trusted(self, active_only=False):
        """Queries at which outputs that use J are compared."""
        return self.margin(active_only) > 2.0 * self.g

    # ---- dense-slot rows ------------------------------------------------------------------------------------------------------
    def rows(self, exact):
        """cols [n, L, 27] (global unknown index or -1), val / mval [n, L, 27], dval / mdval [n, 3, L, 27]; slot s of a row is the
        voxel at floor(q_d) + NBR_OFFSETS[s]; rows of a query whose containing cell is no voxel are 0 (cols -1); cell [n, L] is the
        global index of the containing cell or -1."""
        n, L = self.n, self.depth
        cols = np.full((n, L, 27), -1, np.int64)
        val, mval = np.zeros((n, L, 27)), np.zeros((n, L, 27))
        dval, mdval = np.zeros((n, 3, L, 27)), np.zeros((n, 3, L, 27))
        cell = np.full((n, L), -1, np.int64)
        for d, R in enumerate(self.lv):
            i, j = np.nonzero(R['inslot'] & R['active'][:, None])
            Dij = R['D'][i, j] + 1
            s = Dij[:, 0] * 9 + Dij[:, 1] * 3 + Dij[:, 2]
            cols[i, d, s] = j + self.offsets[d]
            val[i, d, s], mval[i, d, s] = R['Kv'][i, j], R['mKv'][i, j]
            key = 'dKe' if exact else 'dKa'
            for a in range(3):
                dval[i, a, d, s], mdval[i, a, d, s] = R[key][i, a, j], R['m' + key][i, a, j]
            cell[:, d] = np.where(R['active'], R['cell'] + self.offsets[d], -1)
        return dict(cols=cols, val=val, mval=mval, dval=dval, mdval=mdval, cell=cell)

    def take(self, idx):
        """The same reference restricted to the queries ``idx`` (every query stands alone)."""
        sub = object.__new__(FieldRef)
        sub.__dict__.update(self.__dict__)
        sub.p32, sub.n = self.p32[idx], len(np.arange(self.n)[idx])
        sub.lv = [{k: (v if k in ('psi', 'mpsi') else v[idx]) for k, v in R.items()} for R in self.lv]
        return sub


def ratio(got, ref, mag, g, scale=1.0, where=None):
    """max |got - scale ref| / (gamma mag |scale|) over the rows ``where`` (all); a NaN or an error where the bound is 0 gives inf."""
    got, ref, mag = np.asarray(got, F64), np.asarray(ref, F64) * scale, np.asarray(mag, F64) * np.abs(scale)
    if where is not None:
        got, ref, mag = got[where], ref[where], mag[where]
    return bound_ratio(got, ref, g * mag)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name: (what the point cloud is, K, H, depth, seed).  The seeds of the (16, 32) cases are chosen: 64 hidden units per level sit near a
# kink for about 1.5 % of the queries and level, and coarse levels see almost the same t at every query, so a unit that is near 0
# there is near 0 for many queries at once -- most seeds exclude 6 - 12 % of the queries at six levels.
CASES = {
    'one_point':        ('one', 4, 16, 4, 0),          # 27 voxels per level: every rim and every absent neighbour within reach of a query
    'two_clusters':     ('clusters', 16, 32, 4, 21),    # two voxel sets about 6 finest voxels apart: a gap of inactive cells under both supports
    'diagonal_negative': ('diagonal', 4, 32, 4, 2),    # negative coordinates: floor, arithmetic shifts, and u rounds
    'random40':         ('random', 16, 16, 4, 3),
    'depth1_k4':        ('random', 4, 16, 1, 4),
    'depth1_k16':       ('random', 16, 32, 1, 5),
    'depth6_k4':        ('few', 4, 16, MAX_DEPTH, 6),
    'depth6_k16':       ('few', 16, 32, MAX_DEPTH, 30), # the largest dynamic-LDS request of k_evaluate_f_grad
}
INIT_SCALE = 0.5
MIN_FALLBACK = 30           # queries in a cell that is inactive at level 0 under the support of a level-0 voxel
MIN_ON_PLANE = 30           # queries exactly on a face or half-cell plane of level 0
MAX_VOXELS = 1500


def _cloud(kind, rs):
    if kind == 'one':
        return np.array([[0.23, -0.11, 0.07]], F32)
    if kind == 'clusters':
        a = rs.rand(6, 3) * 0.12
        return np.concatenate([a, a[::-1] * 0.9 + [0.62, 0.05, -0.03]]).astype(F32)
    if kind == 'diagonal':
        s = np.linspace(0.0, 1.0, 9)[:, None]
        return (np.array([[-0.93, -0.41, -0.58]]) + s * np.array([[0.5, 0.45, 0.55]])).astype(F32)
    if kind == 'random':
        return ((rs.rand(40, 3) - 0.5) * 0.5).astype(F32)
    if kind == 'few':
        return ((rs.rand(8, 3) - 0.3) * 0.4).astype(F32)
    raise KeyError(kind)


def _queries(oh, xyz, rs):
    """About 300 finite, in-range queries, every family mixed into every prefix."""
    w = F32(VOXEL)
    L0 = oh.levels[0]
    lo, hi = L0.ijk.min(0), L0.ijk.max(0) + 1
    inv_w0 = spec.inv_w0_f32(VOXEL)
    fam = []
    near = xyz[rs.randint(0, len(xyz), 60)] + rs.randn(60, 3) * 0.03
    fam.append(near)
    c, e = 0.5 * (lo + hi) * VOXEL, (hi - lo) * VOXEL
    fam.append(c + (rs.rand(50, 3) - 0.5) * 3.0 * e)                                    # a box 3 x the voxel set: inactive cells, and nothing
    # the rim: inactive level-0 cells next to voxels
    cand = (L0.ijk[rs.randint(0, L0.n, 600)] + 0.5 + (rs.rand(600, 3) - 0.5) * 3.6) * VOXEL
    cand = cand.astype(F32)
    H0, _ = spec.half_index(cand, VOXEL)
    fam.append(cand[L0.lookup((H0 >> 1).astype(np.int32)) < 0][:45])
    # multiples of half a finest voxel in every axis (faces, half-cell planes, corners) over the voxel set and its rim, kept where the
    # fp32 product p lands on the plane exactly; then the same points moved to the next fp32 below
    k = np.stack([rs.randint(2 * lo[a] - 3, 2 * hi[a] + 4, 90) for a in range(3)], 1)
    k[:8] = [[0, 0, 0], [0, 1, 2], [1, 0, -1], [-1, -2, 0], [2, 2, 2], [0, -1, 1], [-2, 0, 0], [1, 1, 1]]
    x = (k * 0.5 * VOXEL).astype(F32)
    exact = ((x * inv_w0).astype(F32) * F32(2.0) == k.astype(F32)).all(1)
    lat = x[exact][:60]
    fam.append(lat)
    fam.append(np.nextafter(lat, F32(-np.inf)))
    fam.append(L0.centers()[rs.randint(0, L0.n, 25)])                                   # voxel centres, fine and coarse
    fam.append(oh.levels[-1].centers()[rs.randint(0, oh.levels[-1].n, 10)])
    fam.append(np.array([[50.0, 50.0, 50.0], [-50.0, 0.05, 0.0], [0.0, 0.0, 50.0]]))     # far from everything
    q = np.concatenate([np.asarray(f, F32) for f in fam]).astype(F32)
    assert np.isfinite(q).all()
    return np.ascontiguousarray(q[rs.permutation(len(q))])


@functools.lru_cache(maxsize=None)
def case(name, dev=None):
    """The inputs of a case -- hierarchy through parity_util.field_inputs (``dev`` None: the oracle side alone) -- and its reference."""
    import parity_util as pu
    kind, K, H, depth, seed = CASES[name]
    rs = np.random.RandomState(100 + seed)
    xyz = _cloud(kind, rs)
    oh, svh, feats, ointerps, net = pu.field_inputs(xyz, dev, K=K, H=H, depth=depth, init_scale=INIT_SCALE, seed=seed)
    assert oh.num_unknowns <= MAX_VOXELS, (name, oh.num_unknowns)
    alpha = rs.randn(oh.num_unknowns).astype(F32)
    q = _queries(oh, xyz, rs)
    levels = [RefLevel(oh.levels[d].ijk, feats[d], it.W1, it.b1, it.W2, it.b2, it.W3, it.b3, alpha[oh.offsets[d]:oh.offsets[d] + oh.levels[d].n])
              for d, it in enumerate(ointerps)]
    ref = FieldRef(levels, q)
    return dict(name=name, K=K, H=H, depth=depth, xyz=xyz, oh=oh, svh=svh, feats=feats, ointerps=ointerps, net=net, alpha=alpha, q=q, ref=ref)


def case_conditions(c):
    """(queries in an inactive level-0 cell with a non-zero level-0 mag, queries exactly on a face or half-cell plane of level 0,
    share of the queries that the ReLU margin excludes -- the larger of the two supports)."""
    ref = c['ref']
    R0 = ref.lv[0]
    fallback = int((~R0['active'] & ((R0['mKv'] @ np.abs(ref.levels[0].alpha)) > 0)).sum())
    p2 = ref.p32.astype(F64) * 2.0
    on_plane = int((p2 == np.floor(p2)).any(1).sum())
    excluded = max(float((~ref.trusted(False)).mean()), float((~ref.trusted(True)).mean()))
    return fallback, on_plane, excluded
