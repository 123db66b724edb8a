"""The structured-matrix family without a GPU: the model of tests/sym_model.py against dense arithmetic (which makes it
trustworthy as the GPU tests' expectation), the cases it builds, the C-ABI of include/mxgpu_sym.h (parsed, exported,
bound beside an untouched mxgpu.h), the classes' validation messages and the transposes that share arrays."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import matrixextra_amd as mx
import sym_model as SM
from matrixextra_amd import _lib, structured

CASES = SM.triplet_cases()


# ---- the model ------------------------------------------------------------------------------------------------------------
def random_triangle(n, uplo, seed, strict=False, repeats=False):
    rng = np.random.default_rng(seed)
    r, c = SM.random_upper(n, 3, seed, diagonal=not strict)
    if repeats and r.size:
        again = rng.integers(0, r.size, r.size // 3)
        r, c = np.concatenate([r, r[again]]), np.concatenate([c, c[again]])
    order = rng.permutation(r.size)
    p, j = SM.csr_of(n, r[order], c[order], uplo, keep_order=True)
    return p, j, rng.integers(1, 50, j.size).astype(np.float64)


@pytest.mark.parametrize("uplo", SM.UPLOS)
@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_model_symmetric_is_T_plus_Tt_minus_diag(n, uplo):
    for seed in range(4):
        p, j, x = random_triangle(n, uplo, seed, repeats=seed % 2 == 1)
        T = SM.to_dense(p, j, x, n)
        assert np.array_equal(T, np.triu(T) if uplo == "U" else np.tril(T))
        op, oj, ox = SM.symmetric_to_general(p, j, x, uplo)
        assert np.array_equal(SM.to_dense(op, oj, ox, n), T + T.T - np.diag(np.diag(T)))
        assert op[-1] == oj.size == ox.size == 2 * j.size - np.count_nonzero(j == SM.rows_of(p))
        pattern = SM.symmetric_to_general(p, j, None, uplo)
        assert np.array_equal(pattern[0], op) and np.array_equal(pattern[1], oj) and pattern[2] is None


@pytest.mark.parametrize("uplo", SM.UPLOS)
def test_model_keeps_sorted_rows_sorted_and_orders_the_halves(uplo):
    n, p, j, _ = SM.case("n300-crosses-the-tiles", uplo, "n", CASES)
    op, oj, _ = SM.symmetric_to_general(p, j, None, uplo)
    for r in range(n):
        row = oj[op[r]:op[r + 1]]
        assert np.all(np.diff(row) > 0)
    # repeats keep their storage order inside the mirrored segment: rows 0 and 1 store (., 2) twice each
    p = np.array([0, 2, 4, 5], dtype=np.int32)
    j = np.array([2, 2, 2, 2, 2], dtype=np.int32)
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    op, oj, ox = SM.symmetric_to_general(p, j, x, "U")
    assert list(op) == [0, 2, 4, 9] and list(oj) == [2, 2, 2, 2, 0, 0, 1, 1, 2] and list(ox) == [1, 2, 3, 4, 1, 2, 3, 4, 5]
    q, k = SM.csr_of(3, [0, 0, 1, 1, 2], [2, 2, 2, 2, 2], "L", keep_order=True)
    op, oj, ox = SM.symmetric_to_general(q, k, x, "L")
    assert list(op) == [0, 2, 4, 9] and list(oj) == [2, 2, 2, 2, 0, 0, 1, 1, 2] and list(ox) == [1, 2, 3, 4, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("uplo", SM.UPLOS)
@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_model_unit_triangular_is_T_plus_I(n, uplo):
    for seed in range(3):
        p, j, x = random_triangle(n, uplo, seed, strict=True)
        T = SM.to_dense(p, j, x, n)
        op, oj, ox = SM.unit_triangular_to_general(p, j, x, "d", uplo)
        assert np.array_equal(SM.to_dense(op, oj, ox, n), T + np.eye(n))
        assert np.array_equal(op, p + np.arange(n + 1)) and oj.size == j.size + n
        at = op[:-1] if uplo == "U" else op[1:] - 1
        assert np.array_equal(oj[at], np.arange(n)) and np.all(ox[at] == 1.0)
        lgl = SM.unit_triangular_to_general(p, j, np.ones(j.size, dtype=np.int32), "l", uplo)
        assert lgl[2].dtype == np.int32 and np.all(lgl[2] == 1) and np.array_equal(lgl[1], oj)


def test_model_refuses_the_wrong_triangle_and_counts_it():
    p, j, x = random_triangle(12, "U", 3)
    assert SM.triangle_check(p, j, "U") == 0
    off = int(np.count_nonzero(j != SM.rows_of(p)))
    assert SM.triangle_check(p, j, "L") == off and SM.triangle_check(p, j, "U", strict=True) == j.size - off > 0
    with pytest.raises(ValueError):
        SM.symmetric_to_general(p, j, x, "L")
    with pytest.raises(ValueError):
        SM.unit_triangular_to_general(p, j, x, "d", "U")


def test_the_cases_are_what_their_names_say():
    assert CASES["n0"][0] == 0 and CASES["n1-diagonal"][0] == CASES["n1-empty"][0] == 1
    n, p, j, x = SM.case("full-first-row", "U", "d", CASES)
    assert p[1] - p[0] == n == 130 > 64
    op, _, _ = SM.symmetric_to_general(p, j, None, "U")
    assert np.all(np.diff(op)[1:] >= np.diff(p)[1:] + 1)                 # every other row gains a mirrored entry
    n, p, j, _ = SM.case("n300-crosses-the-tiles", "L", "n", CASES)
    assert n == 300 and 8500 < j.size < 9500 and j.size > 2 * 4096
    n, p, j, _ = SM.case("all-diagonal", "U", "n", CASES)
    assert np.array_equal(j, np.arange(n)) and SM.symmetric_to_general(p, j, None, "U")[1].size == n
    n, p, j, _ = SM.case("no-diagonal", "U", "n", CASES)
    assert not np.any(j == SM.rows_of(p))
    n, p, j, _ = SM.case("empty-rows-and-columns", "U", "n", CASES)
    op, oj, _ = SM.symmetric_to_general(p, j, None, "U")
    assert np.count_nonzero(np.diff(op) == 0) > 60 and np.unique(oj).size < 20
    for G in SM.GROUP_TARGETS:
        for uplo in SM.UPLOS:
            n, p, j, _ = SM.case(f"lanes-{G}", uplo, "n", CASES)
            assert SM.pick_group(SM.symmetric_to_general(p, j, None, uplo)[1].size / n) == G
    n, p, j, x = SM.case("unsorted-with-repeats", "U", "d", CASES)
    r = SM.rows_of(p)
    assert np.any(np.diff(j)[np.diff(r) == 0] < 0)                       # unsorted rows
    assert np.count_nonzero((j == 7) & (r == 7)) >= 3                    # a repeated diagonal entry
    bits = SM.bits(x)
    for special in (SM.NA_REAL, np.nan, np.inf, -np.inf, -0.0, 0.0):
        assert np.any(bits == SM.bits(np.array([special]))[0])
    assert np.any((x == 0) & (j == r)) and np.any((x == 0) & (j != r))   # explicit zeros on and off the diagonal
    lx = SM.case("unsorted-with-repeats", "U", "l", CASES)[3]
    assert {int(SM.NA_LOGICAL), 0, 1} <= set(lx.tolist())


def test_reference_cases_are_the_dense_matrices_of_the_reference_tests():
    with open(SM.GOLDEN) as f:
        gold = json.load(f)
    sy, tri = gold["sy"], gold["tri"]
    p, j, x = SM.i32(sy["p"]), SM.i32(sy["j"]), np.array(sy["x"], dtype=np.float64)
    op, oj, ox = SM.symmetric_to_general(p, j, x, sy["uplo"])
    assert np.array_equal(SM.to_dense(op, oj, ox, 7), np.array(sy["dense"], dtype=np.float64))
    p, j, x = SM.i32(tri["p"]), SM.i32(tri["j"]), np.array(tri["x"], dtype=np.float64)
    assert np.array_equal(SM.to_dense(p, j, x, 4), np.array(tri["dense"], dtype=np.float64))
    assert SM.triangle_check(p, j, "U") == 0 and SM.triangle_check(p, j, "U", strict=True) == 2


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
NEW = ["mx_csr_symmetric_to_general_begin", "mx_csr_triangle_check", "mx_csr_unit_triangular_to_general_begin",
       "mxd_csr_sym_workspace_bytes", "mxd_csr_symmetric_to_general_count", "mxd_csr_symmetric_to_general_fill",
       "mxd_csr_triangle_check", "mxd_csr_unit_triangular_to_general"]
P, I, I64, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


def test_sym_header_parses_and_is_bound_on_the_same_library():
    with open(_lib.SYM_HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert sorted(h.functions) == NEW == sorted(_lib.SYM_HEADER.functions)
    assert h.constants == {"MX_UPLO_UPPER": 0, "MX_UPLO_LOWER": 1}
    assert (_lib.MX_UPLO_UPPER, _lib.MX_UPLO_LOWER) == (0, 1)
    assert h.functions["mxd_csr_sym_workspace_bytes"] == (SZ, (I, I64))
    assert h.functions["mxd_csr_triangle_check"] == (I, (I, P, P, I64, I, I, P, P, P))
    assert h.functions["mxd_csr_symmetric_to_general_count"] == (I, (I, P, P, I64, I, P, P, P, P))
    assert h.functions["mxd_csr_symmetric_to_general_fill"] == (I, (I, P, P, P, I, I64, I, P, I64, P, P, P, P))
    assert h.functions["mxd_csr_unit_triangular_to_general"] == (I, (I, P, P, P, I, I64, I, P, P, P, P))
    assert h.functions["mx_csr_symmetric_to_general_begin"] == (I, (P, I, P, P, I, I64, I, P, P))
    assert h.functions["mx_csr_unit_triangular_to_general_begin"] == (I, (P, I, P, P, I, I64, I, P, P))
    assert h.functions["mx_csr_triangle_check"] == (I, (P, I, P, I, I, P))
    lib = _lib.load()
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)                                         # exported by libmxgpu.so
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name


def test_mxgpu_h_is_untouched_and_declared_symbols_are_its_own():
    with open(_lib.HEADER_PATH, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "272d0958dbaeeea098083be2d23248951d00c8726dc60aa6e5f6792e8f5b88b3"
    assert not set(NEW) & set(_lib.declared_symbols()) and not set(NEW) & set(_lib.HEADER.functions)
    assert _lib.declared_symbols() == sorted(_lib.HEADER.functions)
    assert not any(k.startswith("MX_UPLO_") for k in _lib.HEADER.constants)


def test_every_device_prototype_states_its_synchronisation():
    with open(_lib.SYM_HEADER_PATH) as f:
        text = f.read()
    waits = {"mxd_csr_triangle_check": "One synchronisation", "mxd_csr_symmetric_to_general_count": "Two synchronisations",
             "mxd_csr_symmetric_to_general_fill": "no synchronisation", "mxd_csr_unit_triangular_to_general": "no synchronisation"}
    assert set(waits) == {n for n, (_, args) in _lib.SYM_HEADER.functions.items() if n.startswith("mxd_") and len(args) > 2}
    for name, words in waits.items():
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert words in comment, name


def test_workspace_holds_what_the_layout_needs():
    lib = _lib.load()
    for n, nnz in ((0, 0), (1, 1), (300, 9000), (10 ** 6, 16 * 10 ** 6)):
        need = 16 + 4 * (n + 1) + 8 * nnz + 4 * n + lib.mxd_csr_transpose_workspace_bytes(nnz) + lib.mxd_scan_workspace_bytes(n)
        assert lib.mxd_csr_sym_workspace_bytes(n, nnz) >= need
        assert lib.mxd_csr_sym_workspace_bytes(n, nnz) <= need + 5 * 16


def test_calls_fail_loudly_on_bad_arguments():
    lib = _lib.load()
    out = C.c_int64(7)
    assert lib.mxd_csr_triangle_check(3, None, None, 0, 2, 0, None, C.byref(out), None) != 0
    assert "uplo must be" in lib.mx_last_error().decode()
    assert lib.mxd_csr_symmetric_to_general_count(-1, None, None, 0, 0, None, None, C.byref(out), None) != 0
    assert "bad size" in lib.mx_last_error().decode()
    assert lib.mxd_csr_symmetric_to_general_fill(2, None, None, None, _lib.MX_F32, 0, 0, None, 0, None, None, None, None) != 0
    assert "unsupported value dtype" in lib.mx_last_error().decode()
    assert lib.mxd_csr_unit_triangular_to_general(2, None, None, None, _lib.MX_F64, 2 ** 31 - 2, 0, None, None, None, None) != 0
    assert "exceeds R's int32 index range" in lib.mx_last_error().decode()
    p = np.array([0, 0], dtype=np.int32)
    assert lib.mx_csr_triangle_check(_lib.ptr(p), 1, None, 5, 0, C.byref(out)) != 0
    with pytest.raises(ValueError, match="invalid 'uplo' field"):
        mx.exports.csr_triangle_check(p, np.zeros(0, np.int32), "X")


# ---- classes --------------------------------------------------------------------------------------------------------------
ALL = [mx.dsRMatrix, mx.lsRMatrix, mx.nsRMatrix, mx.dtRMatrix, mx.ltRMatrix, mx.ntRMatrix, mx.dsCMatrix, mx.dtCMatrix]


def make(cls, n=3, Dim=None, **kw):
    p = np.arange(n + 1, dtype=np.int32)
    j = np.arange(n, dtype=np.int32)
    x = None if cls.value_dtype is None else np.ones(n, dtype=cls.value_dtype)
    return cls(p, j, x, Dim or (n, n), **kw)


@pytest.mark.parametrize("cls", ALL, ids=lambda c: c.r_class)
def test_classes_have_matrix_slots_and_one_common_base(cls):
    X = make(cls)
    assert isinstance(X, mx.StructuredMatrix) and not isinstance(X, (mx.RsparseMatrix, mx.dgCMatrix, mx.TsparseMatrix))
    assert X.r_class == cls.__name__ and X.uplo == "U" and X.Dim == (3, 3) and X.Dimnames == [None, None]
    assert hasattr(X, "diag") == (cls.r_class[1] == "t") and hasattr(X, "j" if cls.layout == "R" else "i")
    assert not hasattr(X, "i" if cls.layout == "R" else "j")
    assert (X.x is None) == (cls.r_class[0] == "n")


@pytest.mark.parametrize("cls", ALL, ids=lambda c: c.r_class)
def test_validation_messages(cls):
    with pytest.raises(mx.MatrixExtraError, match="Matrix type implies square shape, but number of rows and columns differ."):
        mx.check_valid_matrix(make(cls, Dim=(3, 4)))
    with pytest.raises(mx.MatrixExtraError, match="Matrix has invalid 'uplo' field."):
        mx.check_valid_matrix(make(cls, uplo="u"))
    with pytest.raises(mx.MatrixExtraError, match="Matrix has invalid 'uplo' field."):
        mx.check_valid_matrix(make(cls, uplo=["U", "L"]))
    if hasattr(make(cls), "diag"):
        with pytest.raises(mx.MatrixExtraError, match="Matrix has invalid diagonal type."):
            mx.check_valid_matrix(make(cls, diag="X"))
        with pytest.raises(mx.MatrixExtraError, match="Matrix has invalid diagonal type."):     # before uplo, as in the reference
            mx.check_valid_matrix(make(cls, diag=None, uplo="X"))
    X = make(cls)
    X.p = X.p[:-1]
    with pytest.raises(mx.MatrixExtraError, match="'p' doesn't match with dimension"):
        mx.check_valid_matrix(X)
    X = make(cls)
    X.p = X.p + np.int32(1)
    with pytest.raises(mx.MatrixExtraError, match="'p' has bad start/end"):
        mx.check_valid_matrix(X)
    if cls.value_dtype is not None:
        X = make(cls)
        X.x = X.x[:-1]
        with pytest.raises(mx.MatrixExtraError, match="lengths of indices and values differ"):
            mx.check_valid_matrix(X)
    X = make(cls, Dimnames=[["a"], None])
    with pytest.raises(mx.MatrixExtraError, match="Row names of matrix do not match"):
        mx.check_valid_matrix(X)


@pytest.mark.parametrize("cls", [mx.dsRMatrix, mx.dtRMatrix, mx.dsCMatrix, mx.dtCMatrix], ids=lambda c: c.r_class)
def test_t_shallow_shares_arrays_and_flips_uplo(cls):
    X = make(cls, n=4, Dim=(4, 4), Dimnames=[list("abcd"), None], uplo="L")
    T = mx.t_shallow(X)
    twin = {"dsRMatrix": mx.dsCMatrix, "dsCMatrix": mx.dsRMatrix, "dtRMatrix": mx.dtCMatrix, "dtCMatrix": mx.dtRMatrix}
    assert type(T) is twin[cls.r_class] and T.uplo == "U" and T.Dimnames == [None, list("abcd")]
    assert T.p is X.p and T.x is X.x and T.idx is X.idx
    assert hasattr(T, "diag") == hasattr(X, "diag") and getattr(T, "diag", "N") == getattr(X, "diag", "N")
    back = mx.t_shallow(T)
    assert type(back) is cls and back.uplo == "L" and back.idx is X.idx


def test_t_shallow_refuses_the_kinds_without_a_c_twin():
    for cls in (mx.lsRMatrix, mx.nsRMatrix, mx.ltRMatrix, mx.ntRMatrix):
        with pytest.raises(mx.MatrixExtraError, match="column-compressed twin"):
            mx.t_shallow(make(cls))


def test_scalar_route_follows_the_reference_rules():
    """R/slice.R:316-333, 1-based"""
    tri = make(mx.dtRMatrix, n=5)
    assert structured.scalar_route(tri, 4, 2) == ("value", 0.0) and structured.scalar_route(tri, 2, 4) == ("lookup", 2, 4)
    tri.uplo = "L"
    assert structured.scalar_route(tri, 2, 4) == ("value", 0.0) and structured.scalar_route(tri, 4, 2) == ("lookup", 4, 2)
    unit = make(mx.ltRMatrix, n=5, diag="U")
    assert structured.scalar_route(unit, 3, 3) == ("value", 1.0) and structured.scalar_route(unit, 3, 2) == ("value", 0.0)
    sym = make(mx.dsRMatrix, n=5)
    assert structured.scalar_route(sym, 4, 2) == ("lookup", 2, 4) and structured.scalar_route(sym, 2, 4) == ("lookup", 2, 4)
    sym.uplo = "L"
    assert structured.scalar_route(sym, 2, 4) == ("lookup", 4, 2) and structured.scalar_route(sym, 3, 3) == ("lookup", 3, 3)
