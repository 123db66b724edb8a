"""C-ABI surface checks that need no GPU: the library loads, exports every symbol include/mxgpu.h
declares, and compute calls fail loudly (no CPU fallback) when no device is present."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from matrixextra_amd import _lib


def test_library_present_and_loads():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = _lib.load()
    assert lib.mx_abi_version() == 1 == _lib.MXGPU_ABI_VERSION


def test_every_declared_symbol_is_exported():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    assert len(declared) >= 40
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, f"declared in include/mxgpu.h but not exported: {missing}"


def test_every_declared_function_is_bound_from_the_header():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    protos = _lib.HEADER.functions
    assert len(protos) == len(declared) and set(protos) == set(declared)
    returns = {C.c_int, C.c_size_t, C.c_char_p}
    for name in declared:
        restype, argtypes = protos[name]
        fn = getattr(lib, name)
        assert isinstance(fn.argtypes, tuple) and len(fn.argtypes) == len(argtypes), name
        assert tuple(fn.argtypes) == argtypes and fn.restype is restype and restype in returns, name
    with open(_lib.HEADER_PATH) as f:           # the prototypes' own parameter counts, counted here from the text
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in declared:
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, text).group(1).strip()
        assert len(protos[name][1]) == (0 if params in ("", "void") else params.count(",") + 1), name
    assert protos["mxd_scan_workspace_bytes"] == (C.c_size_t, (C.c_int64,))
    assert protos["mx_last_error"] == (C.c_char_p, ())
    assert protos["mx_device_name"] == (C.c_int, (C.c_void_p, C.c_size_t))
    assert protos["mxd_csr_colrange_count"][1][4:7] == (C.c_int, C.c_int, C.c_double)


@pytest.mark.parametrize("header, names", [
    ("int mx_bad(long double x);", ["mx_bad", "long double"]),                  # a parameter type outside the map
    ("int mx_ok(int a);\nvoid mx_bad(int a);", ["mx_bad", "void"]),             # a return type outside the map
    ("int mx_bad(mx_coo_axis axis);", ["mx_bad", "mx_coo_axis"]),               # a struct by value
    ("int mx_ok(int a);\nint mxd_bad(int (*cb)(int));", ["mxd_bad"]),           # a name with `(`, no plain prototype
    ("#define mx_bad(x) (x)\nint mx_ok(int a);\nint y = mx_bad(1);", ["mx_bad"]),
    ("typedef enum { MX_A = 0, MX_B } mx_e;", ["mx_e", "MX_B"]),                # an enumerator without a value
])
def test_the_header_parser_is_strict(header, names):
    with pytest.raises(_lib.MxError) as e:
        _lib.parse_header(header)
    assert all(n in str(e.value) for n in names)


def test_the_header_parser_reads_prototypes_constants_and_structs():
    h = _lib.parse_header("""
        #define MX_TWO 2   /* a comment */
        typedef enum { MX_A = 0, MX_B = 0x10 } mx_e;
        typedef struct { int a, b; const int32_t *p; int64_t n; } mx_s;
        size_t mxd_f(int64_t n, const mx_s *s /* in */, void **out);
        const char *mx_g(void);
    """)
    assert h.functions == {"mxd_f": (C.c_size_t, (C.c_int64, C.c_void_p, C.c_void_p)), "mx_g": (C.c_char_p, ())}
    assert h.constants == {"MX_TWO": 2, "MX_A": 0, "MX_B": 16}
    assert h.structs["mx_s"]._fields_ == [("a", C.c_int), ("b", C.c_int), ("p", C.c_void_p), ("n", C.c_int64)]


def test_wrong_calls_raise_instead_of_running():
    lib = _lib.load()
    with pytest.raises(TypeError):
        lib.mxd_scan_workspace_bytes()                          # too few arguments
    with pytest.raises(C.ArgumentError):
        lib.mxd_scan_workspace_bytes(1.5)
    with pytest.raises(C.ArgumentError):
        lib.mxd_spmm_plan_info(None, 1.5, None)                 # a float where a pointer is expected


def test_64_bit_arguments_and_returns_arrive_whole_unwrapped():
    """mxd_compact_workspace_bytes(2**33) is 16 781 336 bytes (one counter per tile), so it shows that the argument is
    not cut to 32 bits (2**33 would read as 0) but not that the size_t return is whole; the transpose workspace at the
    same count is over 2**31 bytes and shows that."""
    lib = _lib.load()
    big = lib.mxd_compact_workspace_bytes(2**33)
    assert big == lib.mxd_compact_workspace_bytes(C.c_int64(2**33)) == lib.mxd_compact_workspace_bytes(np.int64(2**33))
    assert big != lib.mxd_compact_workspace_bytes(0)
    wide = lib.mxd_csr_transpose_workspace_bytes(2**33)
    assert type(wide) is int and wide >= 2**31
    assert wide == lib.mxd_csr_transpose_workspace_bytes(C.c_int64(2**33))


def test_constants_and_structs_come_from_the_header():
    assert (_lib.MX_F64, _lib.MX_F32, _lib.MX_I32, _lib.MX_LGL, _lib.MX_NONE) == (0, 1, 2, 3, 4)
    assert _lib.MX_OP_AND == 5 and _lib.MX_KEEP_MASK == 3 and _lib.MX_ALIAS_ALL == 2
    assert _lib.MX_DV_OPS == {"*": 0, "^": 1, "/": 2, "%%": 3, "%/%": 4}
    assert _lib.load().mx_abi_version() == _lib.MXGPU_ABI_VERSION
    from matrixextra_amd import exports
    assert exports._RbindInput is _lib.RbindInput and exports.ResultInfo is _lib.ResultInfo
    # sizes of the hand-written ctypes.Structure classes that these replaced
    assert (C.sizeof(_lib.ResultInfo), C.sizeof(_lib.CooAxis), C.sizeof(_lib.RbindInput)) == (32, 40, 48)
    assert [f for f, _ in _lib.ResultInfo._fields_] == ["indptr_len", "nnz", "values_len", "values_dtype",
                                                        "alias_structure"]
    assert [f for f, _ in _lib.CooAxis._fields_] == ["kind", "lo", "hi", "reversed", "nmap", "start", "pos"]
    assert [f for f, _ in _lib.RbindInput._fields_] == ["kind", "indptr", "indices", "values", "nrows", "nnz"]


def test_no_call_argument_is_wrapped_by_hand():
    """In the package, tests/devmem.py and tools/, a ctypes scalar is only made to be handed over by reference."""
    root = os.path.dirname(os.path.dirname(_lib.LIB_PATH))
    files = (glob.glob(os.path.join(root, "matrixextra_amd", "*.py")) + glob.glob(os.path.join(root, "tools", "*.py"))
             + [os.path.join(root, "tests", "devmem.py")])
    assert len(files) > 10
    wrapper = re.compile(r"C\.c_(?:int|int64|size_t|double)\((-?[\d.]+\))?")
    left = []
    for path in files:
        with open(path) as f:
            for k, line in enumerate(f, 1):
                for m in wrapper.finditer(line):
                    # an out-parameter's initialiser: a literal, in an assignment or a return, outside any call
                    before = line[:m.start()]
                    if not (m.group(1) and re.match(r"\s*(return |[\w, ]+ = )", line)
                            and before.count("(") == before.count(")")):
                        left.append(f"{os.path.relpath(path, root)}:{k}: {line.strip()}")
    assert not left, "\n".join(left)


def test_hot_path_export_names_follow_the_reference():
    # one mx_* twin per _MatrixExtra_* routine of the hot path (src/RcppExports.cpp:2233-2242,2290-2298,2333-2343)
    names = set(_lib.declared_symbols())
    for n in ["matmul_dense_csc_numeric", "matmul_dense_csc_float32", "tcrossprod_dense_csr_numeric",
              "tcrossprod_dense_csr_float32", "tcrossprod_csr_dense_numeric", "tcrossprod_csr_dense_float32",
              "matmul_csr_dvec_numeric", "matmul_csr_dvec_integer", "matmul_csr_dvec_logical",
              "matmul_csr_dvec_float32", "check_is_seq", "check_is_rev_seq"]:
        assert "mx_" + n in names
    assert {"mx_csr_elemwise_begin", "mx_copy_csr_rows_begin", "mx_result_finish"} <= names


def test_no_undefined_non_runtime_symbols():
    out = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    undefined = [l.split()[-1] for l in out.splitlines() if l.strip()]
    bad = [u for u in undefined if u.startswith(("mx", "_ZN2mx"))]
    assert not bad, bad


def test_product_does_not_reference_the_oracle():
    root = os.path.dirname(os.path.dirname(_lib.LIB_PATH))
    pkg = os.path.join(root, "matrixextra_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".R")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "mx_oracle" not in text and "from oracle" not in text and "import oracle" not in text, f


@pytest.mark.skipif(_lib.load() is not None and __import__("conftest")._have_gpu(), reason="GPU present")
def test_compute_fails_loudly_without_gpu():
    from matrixextra_amd import exports
    p = np.array([0, 1], dtype=np.int32)
    j = np.array([0], dtype=np.int32)
    x = np.array([1.0])
    with pytest.raises(_lib.MxError):
        exports.tcrossprod_csr_dense_numeric(p, j, x, np.ones((2, 1), order="F"))
    with pytest.raises(_lib.MxError):
        exports.add_csr_elemwise(p, p.copy(), j, j.copy(), x, x.copy(), False)
