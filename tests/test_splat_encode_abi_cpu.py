"""nksr_splat_encode checks its arguments before any launch: the calls below fail cleanly (error code + message) or do nothing on a
machine without a GPU, as the other network entries do in tests/test_abi.py."""
import ctypes as C


def test_splat_encode_argument_errors_without_a_gpu():
    from nksr_amd import _lib
    lib = _lib.lib
    lib.nksr_last_error.restype = C.c_char_p
    big = (C.c_float * 64)()
    A, Z, f1 = C.c_void_p(C.addressof(big)), None, C.c_float(1.0)      # (never dereferenced: every call below returns first)
    full = [A, A, A, A, A, A, A, 3, f1, A, A, A, Z]
    for k in (0, 1, 3, 4, 5, 6, 9, 10, 11):        # every array but the optional normals, alone
        bad = list(full)
        bad[k] = Z
        assert lib.nksr_splat_encode(*bad) != 0 and 'NULL' in lib.nksr_last_error().decode(), k
    for n in (0, -1):                               # no voxel: nothing is looked at
        assert lib.nksr_splat_encode(Z, Z, Z, Z, Z, Z, Z, n, f1, Z, Z, Z, Z) == 0
