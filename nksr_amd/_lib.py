"""ctypes binding of the C-ABI declared in include/nksr_hip.h, READ from that header at import (_cheader.py): the Structure
classes, every argtypes / restype, the constants and EXPORTED are derived, nothing of the ABI is written out here a second time.

The product path has NO CPU fallback: if libnksr_hip.so is missing (and cannot be built)
importing this module raises, and every op raises RuntimeError on a non-GPU tensor.
"""
import ctypes as C
import keyword
import os

import torch

from . import _cheader, build as _build

_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'size_t': C.c_size_t,
            'float': C.c_float, 'double': C.c_double}
assert set(_SCALARS) == set(_cheader.VALUE_TYPES)
_STRUCTS = {}         # 'nksr_fused_op_t' -> FusedOpT


def _ctype(t):
    """A pointer to one of the header's structs is POINTER(ThatStruct); every other pointer is c_void_p (callers pass data_ptr() ints,
    None, byref(...) and ctypes arrays); scalars and nested structs go by their C type."""
    if t.endswith('*'):
        return C.POINTER(_STRUCTS[t[:-1]]) if t[:-1] in _STRUCTS else C.c_void_p
    return _STRUCTS.get(t) or _SCALARS[t]


def _read_header():
    try:
        with open(_build.HEADER) as fh:
            return _cheader.parse(fh.read())
    except OSError as e:
        raise RuntimeError('the ctypes bindings are read from %s, which cannot be opened: %s' % (_build.HEADER, e))


_abi = _read_header()
globals().update((k[len('NKSR_'):], v) for k, v in _abi.consts.items())        # NKSR_MAX_DEPTH -> MAX_DEPTH, ...
for _name, _fields in _abi.structs.items():                                     # nksr_fused_op_t -> FusedOpT, ...
    _cls = ''.join(w.capitalize() for w in _name.split('_')[1:])
    _STRUCTS[_name] = globals()[_cls] = type(_cls, (C.Structure,), {'_fields_': [
        (f + '_' * keyword.iskeyword(f), _ctype(t) * n if n else _ctype(t)) for f, t, n in _fields]})
SiteSetT = SitesetT         # noqa: F821  (nksr_siteset_t: the one name the rule spells differently from its users)


def _load():
    path = _build.LIB
    if _build.needs_build():
        try:
            _build.build_library()
        except Exception as e:  # stale/missing library and no working compiler: fail loudly, never load a stale build silently
            if not os.path.exists(path):
                raise RuntimeError('libnksr_hip.so is missing and could not be built: %s' % e)
            if not os.environ.get('NKSR_ALLOW_STALE_LIB'):
                raise RuntimeError('libnksr_hip.so is older than its sources and the rebuild failed (%s); set '
                                   'NKSR_ALLOW_STALE_LIB=1 to load it anyway' % e)
    return C.CDLL(path)


lib = _load()
for _name, (_ret, _args) in _abi.protos.items():
    _fn = getattr(lib, _name)
    _fn.restype = C.c_char_p if _ret == 'char*' else _ctype(_ret)
    _fn.argtypes = [_ctype(t) for t in _args]
EXPORTED = sorted(_abi.protos)


def check(rc):
    if rc != 0:
        msg = lib.nksr_last_error().decode(errors='replace')
        if 'out of memory' in msg.lower():
            raise MemoryError(msg)
        raise RuntimeError('nksr_hip: %s (code %d)' % (msg, rc))


def ptr(t):
    """Device pointer of a contiguous GPU tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('nksr_amd is MI355X-only: expected a GPU tensor, got device %s' % t.device)
    if not t.is_contiguous():
        raise RuntimeError('expected a contiguous tensor')
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(device):
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("nksr_amd is MI355X-native: device must be 'cuda' (got %s). The CPU restatement of "
                           "this path lives in oracle/ and is test infrastructure only." % device)
    if not torch.cuda.is_available():
        raise RuntimeError('no GPU visible to PyTorch-ROCm')
    return device


def call(name, *args):
    check(getattr(lib, name)(*args))


def with_tmp(name, device, *args_after_tmp):
    """Run a rocPRIM-backed primitive: size query, allocate, run."""
    nbytes = C.c_size_t(0)
    fn = getattr(lib, name)
    check(fn(None, C.byref(nbytes), *args_after_tmp))
    tmp = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=device)
    check(fn(tmp.data_ptr(), C.byref(nbytes), *args_after_tmp))
    return tmp
