"""The C-ABI library loads and exports every symbol include/nksr_hip.h declares (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'nksr_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(nksr_[a-z0-9_]+)\s*\(', src)))


def test_header_symbols_exported():
    from nksr_amd import _lib
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(_lib.lib, n), 'libnksr_hip.so does not export %s' % n
    # and the ctypes table binds exactly the declared entry points
    assert set(_lib.EXPORTED) == set(names), set(_lib.EXPORTED) ^ set(names)


def test_struct_layouts_match_the_header():
    from nksr_amd import _lib
    assert ctypes.sizeof(_lib.LevelT) == 80
    assert ctypes.sizeof(_lib.HierT) == 16 + 6 * 80
    assert ctypes.sizeof(_lib.SiteSetT) == 32 + 2 * 6 * 8 + 16 + 8
    assert ctypes.sizeof(_lib.FusedOpT) == 16 + 8 + 8 * 8 + 8 + 5 * 8 + 3 * 8 + 8 + 8
    assert ctypes.sizeof(_lib.CoarsePrecondT) == 16 + 8 + 14 * 8
    assert ctypes.sizeof(_lib.SegmentsT) == 8 + 3 * 8
    assert _lib.lib.nksr_version() >= 100
    assert _lib.lib.nksr_pcg_workspace_bytes(1000, 50000) >= 4 * 4000


def _flat(v):
    return [x for r in v for x in _flat(r)] if isinstance(v, tuple) else [v]


def test_bindings_match_what_the_compiler_sees(tmp_path):
    """The bindings are read from the header by nksr_amd/_cheader.py, so comparing them with the header proves nothing; the second
    witness is the compiler the library is built with (host only, no device code): sizeof and offsetof of every field of every
    struct, and the value and kind of every numeric macro."""
    import keyword
    import subprocess
    from nksr_amd import _lib, build
    src = re.sub(r'/\*.*?\*/', '', open(build.HEADER).read(), flags=re.S)
    structs = re.findall(r'\}\s*(nksr_\w+_t)\s*;', src)
    macros = re.findall(r'#define (NKSR_\w+)[ \t]+\S', src)
    assert len(structs) == 11 and set(structs) == set(_lib._STRUCTS) and len(macros) >= 15
    lines = ['#include <cstddef>', '#include <cstdio>', '#include <type_traits>', '#include "nksr_hip.h"', 'int main() {']
    for s in structs:
        lines.append('  printf("%s . %%zu 0\\n", sizeof(%s));' % (s, s))
        for f, _ in _lib._STRUCTS[s]._fields_:
            c = f[:-1] if keyword.iskeyword(f[:-1]) else f             # lambda_ -> lambda
            lines.append('  printf("%s %s %%zu %%zu\\n", sizeof(((%s*)0)->%s), offsetof(%s, %s));' % (s, f, s, c, s, c))
    for m in macros:
        v = getattr(_lib, m[len('NKSR_'):])
        if isinstance(v, tuple):            # a brace initialiser: rows, then every element
            inner = '[%d]' % len(v[0]) if isinstance(v[0], tuple) else ''
            lines.append('  { const double a[]%s = %s; const double* p = (const double*)a;' % (inner, m))
            lines.append('    printf("%s %%zu", sizeof(a) / sizeof(a[0])); for (size_t i = 0; i < sizeof(a) / sizeof(double); ++i) '
                         'printf(" %%.17g", p[i]); printf("\\n"); }' % m)
        else:
            lines.append('  printf("%s %%d %%.17g\\n", (int)std::is_integral<decltype(%s)>::value, (double)(%s));' % (m, m, m))
    lines += ['  return 0;', '}']
    (tmp_path / 'probe.cpp').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'probe')
    r = subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-I', os.path.dirname(build.HEADER), str(tmp_path / 'probe.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    seen = 0
    for name, key, *vals in out:
        if name in _lib._STRUCTS:
            cls = _lib._STRUCTS[name]
            want = (ctypes.sizeof(cls), 0) if key == '.' else (getattr(cls, key).size, getattr(cls, key).offset)
            assert (int(vals[0]), int(vals[1])) == want, (name, key, vals, want)
        else:
            v = getattr(_lib, name[len('NKSR_'):])
            if isinstance(v, tuple):
                assert int(key) == len(v) and [float(x) for x in vals] == _flat(v), (name, vals, v)
            else:
                assert bool(int(key)) == isinstance(v, int) and float(vals[0]) == v, (name, key, vals, v)
        seen += 1
    assert seen == len(structs) + sum(len(c._fields_) for c in _lib._STRUCTS.values()) + len(macros)


def test_header_reader_refuses_what_it_does_not_understand():
    import pytest
    from nksr_amd import _cheader
    for text, quoted in (('int nksr_f(const float* x, long n, void* stream);', 'int nksr_f(const float* x, long n, void* stream)'),
                         ('typedef struct { int32_t n; int32_t flags : 3; } nksr_x_t;', 'int32_t flags : 3'),
                         ('int nksr_g(int (*callback)(int), void* stream);', 'int nksr_g(int (*callback)(int), void* stream)'),
                         ('#define NKSR_N sizeof(int)', '#define NKSR_N sizeof(int)'),
                         ('typedef struct { float* a[NKSR_UNDEFINED]; } nksr_y_t;', 'float* a[NKSR_UNDEFINED]')):
        with pytest.raises(_cheader.HeaderError) as e:
            _cheader.parse(text)
        assert quoted in str(e.value), str(e.value)
    ok = _cheader.parse('#define NKSR_K (1ll << 4)\ntypedef struct nksr_s { int32_t a, b[2]; const float* p[NKSR_K]; } nksr_s_t;\n'
                        'const char* nksr_h(const struct nksr_s* s, size_t* n);')
    assert ok.consts == {'NKSR_K': 16} and ok.protos == {'nksr_h': ('char*', ['nksr_s_t*', 'size_t*'])}
    assert ok.structs == {'nksr_s_t': [('a', 'int32_t', None), ('b', 'int32_t', 2), ('p', 'float*', 16)]}


def test_product_refuses_cpu_and_never_imports_oracle():
    import sys
    import pytest
    import torch
    import nksr
    with pytest.raises(RuntimeError):
        nksr.Reconstructor(torch.device('cpu'))
    with pytest.raises(RuntimeError):
        nksr.SparseFeatureHierarchy(0.1, 4, torch.device('cpu'))
    for root, _, files in os.walk(os.path.join(ROOT, 'nksr_amd')):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(root, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', txt, flags=re.M), '%s imports the oracle' % f


def test_api_surface():
    """Names the reference's call sites use."""
    import nksr
    from nksr import Reconstructor, fields, utils  # noqa: F401  (recons_colored_mesh.py:12)
    from nksr.configs import load_checkpoint_from_url  # noqa: F401  (models/nksr_net.py:17)
    from nksr.fields import KernelField, LayerField, NeuralField  # noqa: F401  (models/nksr_net.py:16)
    from nksr.svh import SparseFeatureHierarchy  # noqa: F401  (models/loss.py:12)
    assert callable(nksr.get_estimate_normal_preprocess_fn(64, 85.0))
    import inspect
    sig = inspect.signature(nksr.Reconstructor.reconstruct)
    for kw in ('normal', 'sensor', 'detail_level', 'voxel_size', 'chunk_size', 'preprocess_fn', 'approx_kernel_grad',
               'solver_tol', 'fused_mode'):
        assert kw in sig.parameters
    sig = inspect.signature(fields.BaseField.extract_dual_mesh)
    for kw in ('mise_iter', 'grid_upsample', 'max_points'):
        assert kw in sig.parameters


def test_csr_physical_layouts_roundtrip_on_cpu():
    """include/nksr_hip.h col_format 0 / 1: the host-side decoder (solver.csr_logical) inverts the documented
    tile interleave and the 21-bit column packing."""
    import numpy as np
    import torch
    from nksr_amd import solver
    rng = np.random.default_rng(0)
    nnz = 5000
    cols = rng.integers(0, 1 << 21, nnz).astype(np.int64)
    vals = rng.standard_normal(nnz).astype(np.float32)
    rowptr = torch.tensor([0, nnz], dtype=torch.int32)
    import spmv_layout          # the encoders (tests/spmv_layout.py), shared with the GPU tests that build a CSR by hand
    # format 0: 256-entry tiles, entry m of a tile at 4 (m % 64) + m / 64, int32 columns
    c0, v0 = spmv_layout.encode0(cols, vals)
    assert len(c0) == 8192
    lc, lv = solver.csr_logical(rowptr, torch.from_numpy(c0), torch.from_numpy(v0))
    assert np.array_equal(lc.numpy(), cols) and np.array_equal(lv.numpy(), vals)
    # format 1: 192-entry tiles, entry m at 3 (m % 64) + m / 64, three 21-bit columns per 64-bit word
    c32, v1 = spmv_layout.encode1(cols, vals)
    assert len(c32) == 9216
    packed = spmv_layout.pack21(c32)
    lc, lv = solver.csr_logical(rowptr, torch.from_numpy(packed), torch.from_numpy(v1))
    assert lc.dtype == torch.int32 and np.array_equal(lc.numpy(), cols) and np.array_equal(lv.numpy(), vals)
    assert solver.col_format(torch.from_numpy(packed)) == 1 and solver.col_format(torch.from_numpy(c0)) == 0


def test_c_abi_argument_errors_without_a_gpu():
    """Argument validation happens before any launch: these calls fail cleanly (error code + message) on a
    machine without a GPU, never abort."""
    import ctypes as C
    from nksr_amd import _lib
    lib = _lib.lib
    lib.nksr_last_error.restype = C.c_char_p
    null = C.c_void_p(0)

    def err():
        return lib.nksr_last_error().decode()

    assert lib.nksr_pack_cols21(null, C.c_int64(100), null, null) != 0 and '192' in err()
    assert lib.nksr_spmv_csr(null, null, null, C.c_int32(10), C.c_int64(100), C.c_int(0), null, null, null, null) != 0
    assert 'workspace' in err()
    assert lib.nksr_spmv_plan(null, C.c_int32(10), C.c_int64(100), C.c_int(7), null, null) != 0 and 'col_format' in err()
    assert lib.nksr_spmv_plan(null, C.c_int32(3 << 20), C.c_int64(100), C.c_int(1), null, null) != 0 and '2^21' in err()
    assert lib.nksr_splat_trilinear(null, null, C.c_int(9), null, null, null, null, C.c_int32(1), C.c_float(1.0), null, null, null) != 0
    assert 'channels' in err()
    h = _lib.HierT()
    h.depth = 4
    assert lib.nksr_kernel_rows(C.byref(h), null, C.c_int64(5), C.c_int(0), C.c_float(1.0), null, C.c_int64(0), null, null, null, null, null) != 0 and 'NULL' in err()
    assert lib.nksr_fused_block_counts(C.c_int32(9), C.c_int32(10), C.c_int64(5), null, null, null, null, null) != 0 and 'depth' in err()
    assert lib.nksr_fused_block_counts(C.c_int32(4), C.c_int32(10), C.c_int64(5), null, null, null, null, null) != 0 and 'NULL' in err()
    op = _lib.FusedOpT()
    op.depth, op.M = 4, 10
    assert lib.nksr_fused_apply(C.byref(op), C.c_float(1.0), null, null, null) != 0 and 'NULL' in err()
    assert lib.nksr_hash_build(null, C.c_int32(2), null, null, C.c_int32(4), null) != 0 and 'power of two' in err()
    assert lib.nksr_hash_query(null, C.c_int64(2), null, null, C.c_int32(12), null, null) != 0 and 'power of two' in err()
    # round-2 entry points: argument errors are reported before anything is launched
    hh = _lib.HierT()
    hh.depth = 4
    hh.lv[3].n = 5
    assert lib.nksr_fused_tables(C.byref(hh), C.c_int64(0), null, null, null, null, null, null) != 0 and 'NULL' in err()
    assert lib.nksr_coarse_lambda_max(null, null, null, null, C.c_int32(5), C.c_int(8), null, null, None, C.c_int32(0), null) != 0 and 'NULL' in err()
    # nksr_coarse_precond_apply validates like the solve: NULL pc, 1 .. NKSR_PC_MAX_STEPS steps, ratio > 1, lambda_scale > 0, NULL r / z
    buf = (C.c_float * 256)()
    at = C.cast(buf, C.c_void_p)

    def good_pc():
        pc = _lib.CoarsePrecondT()
        pc.first, pc.n, pc.steps, pc.format, pc.lambda_scale, pc.ratio = 0, 4, 8, 0, 1.1, 40.0
        for f in ('lambda_', 'rowptr', 'cols', 'vals', 'diag', 'work', 'coef'):
            setattr(pc, f, at)
        return pc
    assert 'nksr_coarse_precond_apply' in _lib.EXPORTED
    assert lib.nksr_coarse_precond_apply(None, C.c_int32(1), at, at, null) != 0 and 'NULL' in err()
    for field, value, word in (('steps', 0, 'steps'), ('steps', _lib.PC_MAX_STEPS + 1, 'steps'), ('ratio', 1.0, 'ratio'), ('ratio', 0.5, 'ratio'),
                               ('ratio', float('nan'), 'ratio'), ('lambda_scale', 0.0, 'lambda_scale'), ('n', 0, 'steps'), ('coef', None, 'NULL'),
                               ('diag', None, 'NULL')):
        pc = good_pc()
        setattr(pc, field, value)
        assert lib.nksr_coarse_precond_apply(C.byref(pc), C.c_int32(1), at, at, null) != 0 and word in err(), (field, value, err())
    pc = good_pc()
    assert lib.nksr_coarse_precond_apply(C.byref(pc), C.c_int32(1), null, at, null) != 0 and 'NULL' in err()
    assert lib.nksr_coarse_precond_apply(C.byref(pc), C.c_int32(1), at, null, null) != 0 and 'NULL' in err()
    assert lib.nksr_coarse_precond_apply(C.byref(pc), C.c_int32(0), at, at, null) != 0 and 'nseg' in err()
    assert lib.nksr_coarse_precond_apply(C.byref(pc), C.c_int32(2), at, at, null) != 0 and 'row_seg' in err()      # plain block, two segments
    pc.format = 1
    assert lib.nksr_coarse_precond_apply(C.byref(pc), C.c_int32(1), at, at, null) != 0 and 'packed' in err()
    one = (C.c_float * 8)()
    assert lib.nksr_sdf_from_points(one, one, null, null, null, null, null, C.c_int32(0), C.c_float(1.0), C.c_float(1.0), one, C.c_int64(1), C.c_int(0),
                                    C.c_int(4), C.c_float(0.02), C.c_int(0), one, null, one, null) != 0 and 'nb_points' in err()
    assert lib.nksr_sdf_from_points(one, one, null, null, null, null, null, C.c_int32(0), C.c_float(1.0), C.c_float(1.0), one, C.c_int64(1), C.c_int(8),
                                    C.c_int(4), C.c_float(0.0), C.c_int(0), one, null, one, null) != 0 and 'stdv' in err()
    # the network kernels (csrc/nn.hip, csrc/splat.hip): with n > 0 a NULL array, a channel count the kernel is not built for
    # or a misaligned in / W / out is an argument error before any launch; n <= 0 is a no-op
    big = (C.c_float * 4096)()
    a16 = (C.addressof(big) + 15) & ~15            # a 16-byte aligned host address (never dereferenced: every call below fails first)
    A, odd, Z = C.c_void_p(a16), C.c_void_p(a16 + 4), None
    f1 = C.c_float(1.0)

    def each_null(fn, args, optional=()):
        """``fn(*args)`` must fail with 'NULL' for every pointer argument set to NULL alone (the optional ones excepted)."""
        where = [k for k, a in enumerate(args) if a is A]
        assert where
        for k in where:
            if k in optional:
                continue
            bad = list(args)
            bad[k] = Z
            assert fn(*bad) != 0 and 'NULL' in err(), (fn.__name__, k, err())

    each_null(lib.nksr_sparse_conv3, [A, A, 5, 32, A, A, A, 1, A, Z], optional=(5, 6))
    assert lib.nksr_sparse_conv3(A, A, 5, 16, A, A, Z, 1, A, Z) != 0 and 'f_maps' in err()
    assert lib.nksr_sparse_conv3(odd, A, 5, 32, A, A, Z, 1, A, Z) != 0 and 'aligned' in err()
    assert lib.nksr_sparse_conv3(A, A, 5, 32, odd, A, Z, 1, A, Z) != 0 and 'aligned' in err()
    assert lib.nksr_sparse_conv3(Z, Z, 0, 32, Z, Z, Z, 1, Z, Z) == 0
    each_null(lib.nksr_conv3_wgrad, [A, A, 5, 32, A, A, Z])
    assert lib.nksr_conv3_wgrad(A, A, 5, 31, A, A, Z) != 0 and 'f_maps' in err()
    each_null(lib.nksr_point_mlp, [A, A, 5, f1, 32, A, A, A, A, A, Z])
    assert lib.nksr_point_mlp(A, A, 5, f1, 33, A, A, A, A, A, Z) != 0 and 'f_maps' in err()
    assert lib.nksr_point_mlp(A, A, 5, f1, 32, A, A, A, A, odd, Z) != 0 and 'aligned' in err()
    assert lib.nksr_point_mlp(Z, Z, 0, f1, 32, Z, Z, Z, Z, Z, Z) == 0
    for ch in (32, 5):                              # the half-wave kernel and the generic one
        each_null(lib.nksr_splat_mean, [A, A, ch, A, A, A, A, 3, f1, A, Z])
    for ch in (0, 65):
        assert lib.nksr_splat_mean(A, A, ch, A, A, A, A, 3, f1, A, Z) != 0 and 'channels' in err()
    assert lib.nksr_splat_mean(Z, Z, 32, Z, Z, Z, Z, 0, f1, Z, Z) == 0
    each_null(lib.nksr_splat_trilinear, [A, A, 3, A, A, A, A, 3, f1, A, A, Z])
    assert lib.nksr_splat_trilinear(A, A, 0, A, A, A, A, 3, f1, A, A, Z) != 0 and 'channels' in err()
    each_null(lib.nksr_splat_plane, [A, A, A, A, A, A, 3, f1, A, Z])
    for ch in (32, 5):
        each_null(lib.nksr_pool_children, [A, A, A, 3, ch, A, Z])
    assert lib.nksr_pool_children(A, A, A, 3, 0, A, Z) != 0 and 'positive' in err()
    for ch, src in ((32, A), (8, A), (32, odd)):    # the 16-byte path, the generic one, and the generic one through a misaligned source
        for k, word in ((0, 'NULL'), (1, 'NULL'), (5, 'NULL')):
            args = [src, A, 3, ch, A, A, Z]
            args[k] = Z
            assert lib.nksr_gather_rows(*args) != 0 and word in err(), (ch, k, err())
    assert lib.nksr_gather_rows(A, A, 3, 0, Z, A, Z) != 0 and 'positive' in err()
    each_null(lib.nksr_linear, [A, 3, 32, A, A, 4, A, Z], optional=(4,))
    for cin, cout in ((32, 33), (32, 0), (16, 4)):
        assert lib.nksr_linear(A, 3, cin, A, A, cout, A, Z) != 0 and 'Cout' in err()
    lv = _lib.LevelT()
    lv.n, lv.hcap = 4, 8
    lv.hkeys, lv.hvals = A, A
    assert lib.nksr_udf_decode(None, 0, A, A, 3, f1, f1, 0, A, Z) != 0 and 'null level' in err()
    for k in (2, 3, 8):
        args = [C.byref(lv), 0, A, A, 3, f1, f1, 0, A, Z]
        args[k] = Z
        assert lib.nksr_udf_decode(*args) != 0 and 'NULL' in err(), (k, err())
    for f in ('hkeys', 'hvals'):
        lv2 = _lib.LevelT()
        lv2.n, lv2.hcap, lv2.hkeys, lv2.hvals = 4, 8, A, A
        setattr(lv2, f, None)
        assert lib.nksr_udf_decode(C.byref(lv2), 0, A, A, 3, f1, f1, 0, A, Z) != 0 and 'NULL' in err(), f
    empty = _lib.LevelT()                            # a level without voxels only fills `out`: that one is still checked
    assert lib.nksr_udf_decode(C.byref(empty), 0, Z, Z, 3, f1, f1, 0, Z, Z) != 0 and 'NULL' in err()
    assert lib.nksr_udf_decode(C.byref(empty), 0, Z, Z, 3, f1, f1, 1, A, Z) == 0       # only_unset: nothing to do, nothing launched
    assert lib.nksr_assemble_split_bytes(C.byref(h)) == 0           # no voxels: nothing to split
    with __import__('pytest').raises(RuntimeError):
        _lib.call('nksr_pack_cols21', null, 100, null, null)
