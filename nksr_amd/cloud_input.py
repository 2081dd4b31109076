"""Caller input -> checked device tensors for the cloud tools (``cloud``, ``orient``, ``register``, ``segment``, ``global_register``,
``mls``): what ``mesh_input`` is for the mesh tools.  The cloud tools take GPU tensors only, and say so in one way:
  RuntimeError   what is no floating-point [N, 3] tensor, is not on a GPU, is on another device than its cloud, or is not finite
  ValueError     a number outside its range (``positive``), too many rows
``what`` names the public call in the message (None: the bare argument name).
"""
import torch

from ._lib import require_gpu

INF = float('inf')


def _named(what, name):
    return '%s: %s' % (what, name) if what else name


def rows3(x, what, name='xyz'):
    """x is a floating-point [N, 3] tensor, on whatever device"""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
        raise RuntimeError('%s must be a floating-point [N,3] tensor' % _named(what, name))


def points(x, what, name='xyz', finite=False, max_rows=None):
    """-> x as a float32 contiguous [N, 3] tensor on its GPU: ``rows3``, then ``require_gpu`` (a machine without a GPU reaches the first).
    ``max_rows``: ValueError above it.  ``finite``: ``all_finite``."""
    rows3(x, what, name)
    require_gpu(x.device)
    if max_rows is not None and x.shape[0] > max_rows:
        raise ValueError('%s: %d points, at most %d' % (_named(what, name), x.shape[0], max_rows))
    x = x.to(torch.float32).contiguous()
    if finite:
        all_finite(x, what, name)
    return x


def all_finite(x, what, name='xyz'):
    """one readback (max |x|); RuntimeError for a NaN or an infinity"""
    if x.shape[0] and not float(x.abs().max()) < INF:
        raise RuntimeError('%s: non-finite coordinates' % _named(what, name))


def rows_like(a, n, device, what, name, floating=False, error=RuntimeError):
    """a is a tensor [n, 3] on ``device`` (None: wherever) -- the normals or another per-point attribute of a cloud of n points.
    ``floating``: of a floating-point type as well.  ``error``: what a wrong shape or type raises (``mls`` raises ValueError for
    it, before any device is looked at); a wrong device is a RuntimeError."""
    if not torch.is_tensor(a) or tuple(a.shape) != (n, 3) or (floating and not a.is_floating_point()):
        raise error('%s must be a %s[%d, 3] tensor, one row per point of the cloud (got %s)' % (
            _named(what, name), 'floating-point ' if floating else '', n, tuple(a.shape) if torch.is_tensor(a) else type(a).__name__))
    if device is not None and a.device != device:
        raise RuntimeError('%s is on %s, the cloud on %s' % (_named(what, name), a.device, device))


def positive(value, what, name):
    """-> float(value); ValueError unless 0 < value < inf (a NaN fails both)"""
    value = float(value)
    if not (0.0 < value < INF):
        raise ValueError('%s must be positive and finite (got %r)' % (_named(what, name), value))
    return value


def bbox_centre64(xyz):
    """float64 numpy [3]: the centre of the bounding box of a float32 cloud on the device, 0.5 * (lo + hi) in fp64 -- the point the
    fixed-order sums of ``register.RowSums`` are taken about."""
    from .density import bbox_center
    lo, hi, _ = bbox_center(xyz)
    return 0.5 * (lo.double() + hi.double()).cpu().numpy()
