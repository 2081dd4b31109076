"""The differentiable solve and evaluation of a KernelField (training path, models/nksr_net.py:105-112): the autograd functions of
alpha(normal targets, theta) and f(x; alpha, theta), and the theta vector-Jacobian products behind them -- HIP kernels in the
product (csrc/kfield.hip), the torch statement of the kernel rows (fields/kernel_rows_torch.py) as the reference of the tests."""
import ctypes as C
import os

import torch

from .._lib import ThetaGradT, call, ptr, stream
from . import kernel_rows_torch as krt


def theta_vjp(fld, sets, alpha, lam=None):
    """sum_r g_r . dR'_r / dtheta for the site sets ``sets`` = [(xyz, gradient rows?, sqrt weight, per-row coefficient fn)]:
    the coefficient function maps (u = R' alpha [, v = R' lambda]) of a set to the row factors (a, b) of
    g_r = a_r lambda + b_r alpha  (solve)  or  g_r = a_r alpha  (evaluation)."""
    theta = fld._theta()
    if not theta:
        return []
    if os.environ.get('NKSR_THETA_VJP', 'hip') != 'torch':
        # the product path: HIP kernels.  (The torch statement below is the REFERENCE the tests differentiate -- reached only
        # with NKSR_THETA_VJP=torch; it is never a fallback.)
        if any(torch.is_tensor(sw) for _, _, sw, _ in sets):
            raise RuntimeError('the backward pass of a batched chunk solve (per-site weights) is not supported: train on single fields')
        return theta_vjp_hip(fld, sets, alpha, lam)
    with torch.enable_grad():
        S = torch.zeros((), dtype=torch.float32, device=fld.device)
        for xyz, grad_rows, sw, coeff in sets:
            if xyz is None or xyz.shape[0] == 0:
                continue
            R, idx = krt.rows(fld.svh, fld._interps_in, [f if torch.is_tensor(f) else torch.zeros((0, fld.kdim), device=fld.device)
                                                          for f in fld._feat_in], xyz.to(fld.device, torch.float32), grad_rows,
                              fld.approx_kernel_grad, scale=sw)
            with torch.no_grad():
                Rd = R.detach()
                u = krt.apply_rows(Rd, idx, alpha, grad_rows)
                v = krt.apply_rows(Rd, idx, lam, grad_rows) if lam is not None else None
                a, b = coeff(u, v)
                m = (idx >= 0).to(torch.float32)
                ag = alpha[idx.clamp(min=0)] * m                                   # [n, L, 27]
                lg = lam[idx.clamp(min=0)] * m if lam is not None else None
                if grad_rows:                                                      # rows [n, 3, L, 27], factors [n, 3]
                    g = (a[..., None, None] * lg[:, None] if lg is not None else 0.0) + b[..., None, None] * ag[:, None]
                else:
                    g = (a[:, None, None] * lg if lg is not None else 0.0) + b[:, None, None] * ag
            S = S + (R * g).sum()
        grads = torch.autograd.grad(S, theta, allow_unused=True)
    return [gr if gr is not None else torch.zeros_like(t) for gr, t in zip(grads, theta)]


def theta_vjp_hip(fld, sets, alpha, lam=None):
    """The same sum as _theta_vjp in HIP (csrc/kfield.hip: nksr_kernel_rows_vjp + nksr_voxel_psi_vjp): the per-row factors
    from two field evaluations with the rows' support (u = R' alpha, v = R' lambda are f / grad f at the sites), then one
    thread per (site, level) recomputes its row's forward and pushes the cotangents into the basis features (trilinear
    stencil), the neighbours' psi and the interpolator weights; psi_j = f_j + MLP(f_j) is taken back per voxel.  Returns
    the gradients in the order of ``_theta()``.  (kernel_rows_torch.py stays the reference the tests differentiate.)"""
    dev, L, K = fld.device, fld.svh.depth, fld.kdim
    al = alpha.detach().to(dev, torch.float32).contiguous()
    lm = lam.detach().to(dev, torch.float32).contiguous() if lam is not None else None
    gfeat = [torch.zeros_like(fld._feat[d]) for d in range(L)]
    gpsi = [torch.zeros_like(fld._feat[d]) for d in range(L)]
    gmlp = [torch.zeros_like(fld._mlp[d]) for d in range(L)]
    tg = ThetaGradT()
    for d in range(L):
        tg.gfeat[d] = ptr(gfeat[d]) if gfeat[d].numel() else None
        tg.gpsi[d] = ptr(gpsi[d]) if gpsi[d].numel() else None
        tg.gmlp[d] = ptr(gmlp[d])
    with torch.no_grad():
        for xyz, grad_rows, sw, coeff in sets:
            if xyz is None or xyz.shape[0] == 0:
                continue
            xs = xyz.detach().to(dev, torch.float32).contiguous()
            ra = fld._evaluate_raw(al, xs, bool(grad_rows), active_only=True)
            u = (ra.gradient if grad_rows else ra.value) * float(sw)
            v = None
            if lm is not None:
                rl = fld._evaluate_raw(lm, xs, bool(grad_rows), active_only=True)
                v = (rl.gradient if grad_rows else rl.value) * float(sw)
            a, b = coeff(u, v)
            ca = a.to(dev, torch.float32).contiguous() if (a is not None and lm is not None) else None
            cb = b.to(dev, torch.float32).contiguous() if b is not None else None
            if ca is None and cb is None:
                continue
            call('nksr_kernel_rows_vjp', C.byref(fld._hier), ptr(xs), xs.shape[0], int(bool(grad_rows)), int(fld.approx_kernel_grad), float(sw),
                 ptr(ca), ptr(cb), ptr(al), ptr(lm) if ca is not None else None, C.byref(tg), stream())
        for d in range(L):
            n_d = fld._feat[d].shape[0]
            if n_d:
                call('nksr_voxel_psi_vjp', ptr(fld._feat[d]), n_d, K, fld.hidden, ptr(fld._mlp[d]), ptr(gpsi[d]), ptr(gfeat[d]), ptr(gmlp[d]), stream())
    out = [gfeat[d].to(f.device, f.dtype) for d, f in enumerate(fld._feat_in) if torch.is_tensor(f) and f.requires_grad]
    H = fld.hidden
    sizes = [H * K, H, H * H, H, K * H, K]
    for d, m in enumerate(fld._interps_in):
        if isinstance(m, torch.nn.Module):
            parts = dict(zip(('W1', 'b1', 'W2', 'b2', 'W3', 'b3'), torch.split(gmlp[d], sizes)))
            for name, q in m.named_parameters():
                if q.requires_grad:
                    out.append(parts[name].reshape(q.shape).to(q.device, q.dtype))
    return out


class _SolveFunction(torch.autograd.Function):
    """alpha(normal targets, theta) for the system of the field's last solve:  A(theta) alpha = b(theta, n),
    A = sum_r R'_r^T R'_r + reg I,  b = sum_r R'_r t'_r  (R' = sqrt(w) R, t' = sqrt(w) n on the gradient rows, 0 on the position rows).
    With A lambda = dL/dalpha:  dL/dn = w_n Q lambda  ((Q lambda)[k, a] is d/dx_a of the kernel field with coefficients lambda at
    normal site k -- one PCG solve and one gradient evaluation) and
    dL/dtheta = sum_r dR'_r . [(t'_r - u_r) lambda - v_r alpha],  u = R' alpha, v = R' lambda  (KernelField._theta_vjp)."""

    @staticmethod
    def forward(ctx, field, alpha, pos_xyz, normal_xyz, normal_value, pos_weight, normal_weight, *theta):
        ctx.field, ctx.pos_xyz, ctx.normal_xyz = field, pos_xyz, normal_xyz
        ctx.pos_weight, ctx.normal_weight, ctx.n_theta = pos_weight, normal_weight, len(theta)
        ctx.normal_value = normal_value.detach()
        return alpha.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_alpha):
        fld = ctx.field
        lam = fld._solve_system(g_alpha.to(torch.float32))
        g_n = None
        if ctx.normal_xyz is not None and ctx.normal_value.numel():
            g_n = ctx.normal_weight * fld._evaluate_raw(lam, ctx.normal_xyz, True).gradient
        g_theta = []
        if ctx.n_theta:
            alpha = fld.alpha.detach()
            swp, swn = ctx.pos_weight ** 0.5, ctx.normal_weight ** 0.5
            tn = ctx.normal_value.to(fld.device, torch.float32) * swn if ctx.normal_value.numel() else None
            sets = [(ctx.pos_xyz, False, swp, lambda u, v: (-u, -v)),
                    (ctx.normal_xyz, True, swn, lambda u, v: ((tn - u) if tn is not None else -u, -v))]
            g_theta = fld._theta_vjp(sets, alpha, lam)
        return (None, None, None, None, g_n, None, None) + tuple(g_theta)


class _EvaluateFunction(torch.autograd.Function):
    """f(x) and grad f(x) as functions of alpha (linear) and theta: dL/dalpha = G_x^T g_f + Q_x^T g_grad, the set-up pass of the
    matrix-free operator over the kernel rows of the query points; dL/dtheta = sum_x dR_x . (g alpha) (KernelField._theta_vjp).
    Query points are not differentiated.  Support: the kernel rows exist only where the query lies in an active cell of the
    level, so the FORWARD of this (training) path is evaluated with the same support (nksr_evaluate_f active_only) -- the
    inference path (no autograd) also adds the levels whose neighbours a query outside every active cell still touches."""

    @staticmethod
    def forward(ctx, field, alpha, xyz, want_grad, max_points, *theta):
        ctx.field, ctx.xyz, ctx.want_grad, ctx.n_theta = field, xyz, want_grad, len(theta)
        ctx.alpha = alpha.detach()
        res = field._evaluate_raw(alpha, xyz, want_grad, max_points, active_only=True)
        g = res.gradient if want_grad else torch.zeros((0, 3), dtype=torch.float32, device=res.value.device)
        return res.value, g

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_f, g_grad):
        fld = ctx.field
        if ctx.xyz.shape[0] == 0:           # no queries: zero gradients
            th = fld._theta()[:ctx.n_theta]
            return (None, torch.zeros_like(ctx.alpha), None, None, None) + tuple(torch.zeros_like(q) for q in th)
        use_g = ctx.want_grad and g_grad is not None and g_grad.numel() > 0
        g_f = g_f if g_f is not None else torch.zeros(ctx.xyz.shape[0], device=fld.device)
        op = fld.fused_operator(ctx.xyz, ctx.xyz if use_g else None, g_grad if use_g else None, 1.0, 1.0, pos_value=g_f)
        b, _ = fld.fused_rhs_diag(op, 0.0)
        g_theta = []
        if ctx.n_theta:
            sets = [(ctx.xyz, False, 1.0, lambda u, v: (None, g_f.to(torch.float32)))]
            if use_g:
                sets.append((ctx.xyz, True, 1.0, lambda u, v: (None, g_grad.to(torch.float32))))
            g_theta = fld._theta_vjp(sets, ctx.alpha, None)
        return (None, b, None, None, None) + tuple(g_theta)
