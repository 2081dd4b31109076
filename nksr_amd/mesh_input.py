"""Caller input (numpy arrays or tensors, on any device) -> checked device tensors, for ``metrics``, ``mesh_query`` and ``mesh_topology``.
Points are recentred in float64 and rounded to float32 once (``bbox_centre``, ``recentre``).  ``faces`` reads in two ways:
  cast_float=True,  check_range=True    MeshEvaluator, sample_surface, MeshQuery: any dtype is an index (a mesh stored as floats
                                        loads as it is), and an index outside [0, V) is an error
  cast_float=False, check_range=False   MeshTopology: float and bool faces are an error, and an index outside [0, V) passes, to be
                                        counted there as an invalid face
"""
import numpy as np
import torch

from ._lib import require_gpu


def gpu_device(device=None, like=None):
    """The GPU to work on: ``device``, else the device of ``like`` when that is a GPU tensor, else the current one."""
    if device is None:
        device = like.device if isinstance(like, torch.Tensor) and like.is_cuda else 'cuda'
    device = require_gpu(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def rows3(x, name):
    shape = tuple(x.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError('%s: expected an [N, 3] array, got shape %s' % (name, shape))


def bbox_centre(x):
    """float64 centre of the bounding box of x (numpy array or tensor) as a numpy [3] array."""
    x = x.detach() if isinstance(x, torch.Tensor) else np.asarray(x)
    rows3(x, 'target')
    if x.shape[0] == 0:
        raise ValueError('the target cloud is empty')
    if isinstance(x, torch.Tensor):
        lo, hi = x.amin(0).double().cpu().numpy(), x.amax(0).double().cpu().numpy()
    else:
        lo, hi = x.min(0).astype(np.float64), x.max(0).astype(np.float64)
    return 0.5 * (lo + hi)


def recentre(x, centre, dev, name):
    """float32 copy of x - centre on dev, the difference taken in float64."""
    x = x.detach() if isinstance(x, torch.Tensor) else np.asarray(x)
    rows3(x, name)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        out = (x.to(dev, torch.float64) - torch.from_numpy(centre).to(dev)).to(torch.float32)
    else:                       # (a CPU tensor goes the numpy way)
        out = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64) - centre, dtype=np.float32)).to(dev)
    out = out.contiguous()
    if out.numel() and not bool(torch.isfinite(out).all()):
        raise ValueError('%s: non-finite coordinates' % name)
    return out


def normals32(n, count, dev, name):
    if n is None:
        return None
    rows3(n, name)
    t = n.detach() if isinstance(n, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(n, np.float32)))
    t = t.to(dev, torch.float32).contiguous()
    if t.shape[0] != count:
        raise ValueError('%s: %d rows for %d points' % (name, t.shape[0], count))
    if t.numel() and not bool(torch.isfinite(t).all()):
        raise ValueError('%s: non-finite values' % name)
    return t


def faces(f, nv, dev, *, cast_float, check_range):
    """[F, 3] int32 / int64 faces on dev, read in one of the two ways above (other dtypes become int64, no faces become [0, 3])."""
    t = f.detach() if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(f)))
    if t.dtype not in (torch.int32, torch.int64):
        if not cast_float and (t.dtype.is_floating_point or t.dtype == torch.bool):
            raise ValueError('faces: expected integer indices, got %s' % t.dtype)
        t = t.to(torch.int64)
    if t.numel() == 0:
        return t.reshape(0, 3).to(dev)
    rows3(t, 'faces')
    t = t.to(dev).contiguous()
    if check_range and (int(t.min()) < 0 or int(t.max()) >= nv):
        raise ValueError('faces: vertex index outside [0, %d)' % nv)
    return t


def is64(f):                # the ``faces_int64`` argument of the C entry points
    return int(f.dtype == torch.int64)
