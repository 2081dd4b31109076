"""Residency of parked fields: borrowing one onto the compute device for a block, spilling one from host memory to disk."""
import contextlib
import os
import uuid

import torch


@contextlib.contextmanager
def borrowed(obj, device):
    """A PARKED field (its tensors live on ``chunk_tmp_device`` / were moved by ``to_('cpu')``: NKSR-USAGE.md:150-167) made usable on
    ``device`` for the duration of the block: ``to_()`` replaces the object's tensors by copies on ``device``; on exit the references
    to the parked tensors are put back and the copies die.  Nothing travels back -- evaluation and meshing do not change a field.
    ``obj``: a KernelField (with its hierarchy and mask) or a SparseFeatureHierarchy."""
    device = torch.device(device)

    def _norm(d):      # 'cuda' names the CURRENT device: compare full (type, index) pairs -- a field parked on another GPU is NOT resident
        d = torch.device(d)
        return (d.type, d.index if d.index is not None else (torch.cuda.current_device() if d.type == 'cuda' and torch.cuda.is_available() else 0))
    if _norm(obj.device) == _norm(device):
        yield obj
        return
    objs = [obj]
    for o in (getattr(obj, 'svh', None), getattr(obj, 'mask_field', None), getattr(getattr(obj, 'mask_field', None), 'svh', None)):
        if o is not None and all(o is not q for q in objs):
            objs.append(o)
    saved = [(o, dict(o.__dict__)) for o in objs]
    try:
        obj.to_(device)
        yield obj
    finally:
        for o, d in saved:
            o.__dict__.clear()
            o.__dict__.update(d)


def spill_to_disk(field, directory):
    """A field PARKED on the host (``to_('cpu')``) moved on to DISK: every tensor of the field, its hierarchy and its mask is replaced
    by a file-backed copy (``torch.from_file(..., shared=True)``, one file per tensor under ``directory``, unlinked at once: the
    mapping keeps the blocks until the tensor dies, nothing is left behind).  The host then holds reclaimable page cache instead of
    anonymous memory, and ``borrowed()`` pages a part in when evaluation / meshing visits it -- the out-of-core flow of
    NKSR-USAGE.md:150-167 for scenes whose solved chunks exceed host memory too.  Returns the bytes written."""
    os.makedirs(directory, exist_ok=True)
    total = 0
    seen = set()

    def move(t):
        nonlocal total
        if not torch.is_tensor(t) or t.device.type != 'cpu' or t.numel() == 0 or t.dtype == torch.bool:
            return t
        path = os.path.join(directory, 'nksr_spill_%s.bin' % uuid.uuid4().hex)
        flat = torch.from_file(path, shared=True, size=t.numel(), dtype=t.dtype)
        flat.copy_(t.reshape(-1))
        os.unlink(path)
        total += t.numel() * t.element_size()
        return flat.view(t.shape)

    def walk(o):
        if o is None or id(o) in seen or not hasattr(o, '__dict__'):
            return
        seen.add(id(o))
        for k, v in list(o.__dict__.items()):
            if torch.is_tensor(v):
                o.__dict__[k] = move(v)
            elif isinstance(v, (list, tuple)) and v and all(torch.is_tensor(x) or x is None for x in v):
                o.__dict__[k] = type(v)(move(x) for x in v)
            elif isinstance(v, (list, tuple)):
                for x in v:
                    if type(x).__module__.startswith('nksr_amd'):
                        walk(x)
            elif type(v).__module__.startswith('nksr_amd') and not isinstance(v, type):
                walk(v)
    if field.device.type != 'cpu':
        raise RuntimeError('spill_to_disk: park the field on the host first (field.to_("cpu"))')
    walk(field)
    return total
