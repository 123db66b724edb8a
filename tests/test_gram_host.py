"""The one-triangle Gram product before a device call: include/mxgpu_gram.h as the binding reads it, the failures on bad
arguments, what the one-argument crossprod / tcrossprod of matmul.py decide under options["mxgpu.spgemm_route"] together
with options["mxgpu.gram_symmetric"] (the flags of the one export call, the class, uplo, Dim and Dimnames of the
result), and device.spgemm(..., uplo=...) / device.gram on the recording fake of tests/device_trace.py.
exports.csr_gram is replaced by a numpy stand-in, so no GPU is needed; without both options it is never reached."""
import ctypes as C

import numpy as np
import pytest

import device_trace as T
import matrixextra_amd as mx
from conftest import csr_to_dense
from matrixextra_amd import _lib, device as D, exports as G, matmul
from matrixextra_amd.matrices import options
from matrixextra_amd.structured import check_valid_structured, dsCMatrix, dsRMatrix
from test_spgemm_host import M_, K_, dense_to_csr, int_dense, operand

NEW = ["mx_csr_gram_begin", "mxd_csr_spgemm_tri_count", "mxd_csr_spgemm_tri_fill"]
P, I, I64 = C.c_void_p, C.c_int, C.c_int64
F64, F32, NONE = _lib.MX_F64, _lib.MX_F32, _lib.MX_NONE
U, L = _lib.MX_UPLO_UPPER, _lib.MX_UPLO_LOWER


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_gram_header_parses_to_three_prototypes_bound_on_the_same_library():
    with open(_lib.GRAM_HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert sorted(h.functions) == NEW == sorted(_lib.GRAM_HEADER.functions)
    assert h.constants == {} and h.structs == {}                        # mx_uplo stays where it is, in mxgpu_sym.h
    assert h.functions["mxd_csr_spgemm_tri_count"] == (I, (I, I, I, P, P, I64, P, P, I64, I, I, P, P, P, P, P))
    assert h.functions["mxd_csr_spgemm_tri_fill"] == (I, (I, I, I, P, P, P, I, P, P, P, I, I, I, P, P, P, P, P))
    assert h.functions["mx_csr_gram_begin"] == (I, (P, I, I, P, P, I, I, I, P, P))
    lib = _lib.load()
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)                                         # exported by libmxgpu.so
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name
    # the device prototypes are those of mxgpu_spgemm.h with (uplo, b_sorted) behind the operands
    for tri, plain, at in (("mxd_csr_spgemm_tri_count", "mxd_csr_spgemm_count", 9),
                           ("mxd_csr_spgemm_tri_fill", "mxd_csr_spgemm_fill", 11)):
        args = _lib.SPGEMM_HEADER.functions[plain][1]
        assert h.functions[tri][1] == args[:at] + (I, I) + args[at:]


def test_the_other_headers_keep_their_function_sets():
    others = (_lib.HEADER, _lib.REDUCE_HEADER, _lib.SYM_HEADER, _lib.TPROD_HEADER, _lib.SPGEMM_HEADER)
    assert not any(set(NEW) & set(h.functions) for h in others) and not set(NEW) & set(_lib.declared_symbols())
    assert sorted(_lib.SPGEMM_HEADER.functions) == ["mx_csr_spgemm_begin", "mxd_csr_spgemm_count", "mxd_csr_spgemm_fill",
                                                    "mxd_csr_spgemm_limits", "mxd_csr_spgemm_workspace_bytes"]
    assert sorted(_lib.TPROD_HEADER.functions) == ["mx_csr_tmatmul_dense", "mx_csr_tmatvec", "mxd_csr_transpose_by_order",
                                                   "mxd_segment_dot"]
    assert {"MX_UPLO_UPPER": 0, "MX_UPLO_LOWER": 1}.items() <= _lib.SYM_HEADER.constants.items()
    assert _lib.HEADER.constants["MXGPU_ABI_VERSION"] == _lib.load().mx_abi_version()


def test_every_device_prototype_states_its_synchronisation():
    with open(_lib.GRAM_HEADER_PATH) as f:
        text = f.read()
    for name, waits in (("mxd_csr_spgemm_tri_count", True), ("mxd_csr_spgemm_tri_fill", False)):
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == waits and ("no synchronisation" in comment) == (not waits), name
    at = text.index("int mxd_csr_spgemm_tri_count(")
    assert "products inside the window" in text[text.rindex("/*", 0, at):at]     # what *products_host holds is said


def test_calls_fail_loudly_on_bad_arguments_before_any_device_work():
    lib = _lib.load()
    err = lambda: lib.mx_last_error().decode()                          # noqa: E731
    p = np.zeros(3, np.int32)
    res, info = C.c_void_p(), _lib.ResultInfo()
    begin = lambda *a: lib.mx_csr_gram_begin(*a, C.byref(res), C.byref(info))       # noqa: E731
    assert lib.mx_csr_gram_begin(_lib.ptr(p), 2, 2, None, None, F64, 0, U, None, None) != 0 and "null pointer" in err()
    assert begin(None, 2, 2, None, None, F64, 0, U) != 0 and "null pointer" in err()
    assert begin(_lib.ptr(p), 2, -2, None, None, F64, 1, L) != 0 and "negative dimension" in err()
    assert begin(_lib.ptr(p), -2, 2, None, None, F64, 1, L) != 0 and "negative dimension" in err()
    assert begin(_lib.ptr(p), 2, 2, None, None, F32, 0, U) != 0 and "unsupported value dtype" in err()
    for bad in (2, -1):
        assert begin(_lib.ptr(p), 2, 2, None, None, F64, 0, bad) != 0 and "uplo" in err()
    bad_p = np.array([0, 1, -1], np.int32)
    assert begin(_lib.ptr(bad_p), 2, 2, None, None, F64, 0, U) != 0 and "bad index pointer" in err()
    one = np.array([0, 1, 1], np.int32)
    assert begin(_lib.ptr(one), 2, 2, None, None, NONE, 0, U) != 0 and "null pointer" in err()        # entries, no indices
    assert begin(_lib.ptr(one), 2, 2, _lib.ptr(p), None, F64, 0, U) != 0 and "null pointer" in err()  # no values
    assert res.value is None
    # the device entries: uplo and the sizes first, with every pointer null
    assert lib.mxd_csr_spgemm_tri_count(1, 1, 1, None, None, 0, None, None, 0, 2, 0, None, None, None, None, None) != 0
    assert "uplo" in err()
    assert lib.mxd_csr_spgemm_tri_count(1, -1, 1, None, None, 0, None, None, 0, U, 0, None, None, None, None, None) != 0
    assert "negative dimension" in err()
    assert lib.mxd_csr_spgemm_tri_fill(1, 1, 1, None, None, None, F64, None, None, None, F64, 7, 0, None, None, None, None,
                                       None) != 0 and "uplo" in err()
    assert lib.mxd_csr_spgemm_tri_fill(1, 1, -1, None, None, None, F64, None, None, None, F64, L, 0, None, None, None, None,
                                       None) != 0 and "negative dimension" in err()
    with pytest.raises(ValueError, match="indptr and dims disagree"):
        G.csr_gram(p, np.zeros(0, np.int32), None, (3, 2), False, "U")
    with pytest.raises(ValueError, match="invalid 'uplo'"):
        G.csr_gram(p, np.zeros(0, np.int32), None, (2, 2), False, "X")


# ---- the mirror --------------------------------------------------------------------------------------------------------
# (trans, uplo of the mask, class) of the export call, written out: a CSC operand's arrays are the CSR of its transpose,
# and the rows of the lower mask, read as columns, are the upper triangle
FLAGS = {("crossprod", "R"): (True, "U", dsRMatrix), ("crossprod", "C"): (False, "L", dsCMatrix),
         ("tcrossprod", "R"): (False, "U", dsRMatrix), ("tcrossprod", "C"): (True, "L", dsCMatrix)}
CALL = {"crossprod": mx.crossprod, "tcrossprod": mx.tcrossprod}
DENSE = {"crossprod": lambda X: X.T @ X, "tcrossprod": lambda X: X @ X.T}


@pytest.fixture
def calls(monkeypatch):
    """exports.csr_gram records its arguments and answers in numpy: the triangle of the dense Gram product, with the
    symbolic pattern; exports.csr_spgemm must not be reached; the sortedness check answers in numpy too"""
    seen = []

    def csr_gram(p, j, x, dims, trans, uplo):
        seen.append((p, j, x, tuple(dims), trans, uplo))
        assert p.size == dims[0] + 1 and uplo in ("U", "L")
        assert all(np.all(np.diff(j[p[r]:p[r + 1]]) > 0) for r in range(p.size - 1)), "the export is given sorted rows"
        V = csr_to_dense(p, j, np.ones(j.size) if x is None else np.where(x == mx.NA_INTEGER, np.nan, x), dims[1])
        S = csr_to_dense(p, j, np.ones(j.size), dims[1])
        with np.errstate(invalid="ignore"):
            V = np.nan_to_num(V)
            out, pattern = (V.T @ V, S.T @ S) if trans else (V @ V.T, S @ S.T)
        tri = np.triu if uplo == "U" else np.tril
        rp, rj, rx = dense_to_csr(out, keep=tri(pattern != 0))
        return dict(indptr=rp, indices=rj, values=rx)

    def no_spgemm(*a):
        raise AssertionError("the general product was called")

    monkeypatch.setattr(G, "csr_gram", csr_gram)
    monkeypatch.setattr(G, "csr_spgemm", no_spgemm)
    monkeypatch.setattr(G, "check_indices_are_sorted",
                        lambda p, j: all(np.all(np.diff(j[p[r]:p[r + 1]]) > 0) for r in range(p.size - 1)))
    monkeypatch.setattr(G, "csr_triangle_check", lambda p, j, uplo, strict=False: int(sum(
        (j[p[r]:p[r + 1]] < r).sum() if uplo == "U" else (j[p[r]:p[r + 1]] > r).sum() for r in range(p.size - 1))))
    return seen


@pytest.fixture
def both():
    options["mxgpu.spgemm_route"] = True
    options["mxgpu.gram_symmetric"] = True
    yield
    options.pop("mxgpu.spgemm_route", None)
    options.pop("mxgpu.gram_symmetric", None)


def upper_dense(out):
    """the stored triangle of a symmetric result as a dense upper-triangular matrix"""
    n = out.Dim[0]
    if isinstance(out, dsCMatrix):
        return csr_to_dense(out.p, out.i, out.x, n).T
    return csr_to_dense(out.p, out.j, out.x, n)


def test_gram_flags_are_the_four_cases_written_out():
    for (signature, layout), want in FLAGS.items():
        assert matmul.gram_flags(signature, layout) == want
    assert len({matmul.gram_flags(s, l)[0] for s in CALL for l in "RC"}) == 2


@pytest.mark.parametrize("signature,layout", sorted(FLAGS))
def test_every_signature_and_layout(calls, both, signature, layout):
    D_ = int_dense((M_, K_), 21)
    X = operand(D_, layout, "x")
    out = CALL[signature](X)
    (p, j, x, dims, trans, uplo), = calls
    want_trans, want_uplo, cls = FLAGS[signature, layout]
    assert (trans, uplo) == (want_trans, want_uplo)
    idx = X.j if layout == "R" else X.i
    assert p is X.p and j is idx and x is X.x and dims == (X.Dim if layout == "R" else X.Dim[::-1])   # the arrays as they are
    want = DENSE[signature](D_)
    n = want.shape[0]
    assert type(out) is cls and out.uplo == "U" and out.Dim == (n, n)
    assert np.array_equal(upper_dense(out), np.triu(want))
    names = X.Dimnames[1] if signature == "crossprod" else X.Dimnames[0]
    assert out.Dimnames == [names, names]
    check_valid_structured(out)                                          # the triangle check answers in numpy here


def test_logical_and_pattern_operands_keep_their_values_for_the_export(calls, both):
    D_ = int_dense((M_, K_), 22)
    p, j, _ = dense_to_csr(D_)
    xl = np.where(np.arange(j.size) % 3 == 0, mx.NA_INTEGER, 1).astype(np.int32)
    Lg, N = mx.lgRMatrix(p, j, xl, (M_, K_)), mx.ngRMatrix(p, j, None, (M_, K_))
    out = mx.crossprod(Lg)
    assert calls[-1][2] is Lg.x and calls[-1][2].dtype == np.int32 and type(out) is dsRMatrix and out.x.dtype == np.float64
    out = mx.tcrossprod(N)
    assert calls[-1][2] is None and calls[-1][4:] == (False, "U") and type(out) is dsRMatrix
    S = (D_ != 0).astype(float)
    assert np.array_equal(upper_dense(out), np.triu(S @ S.T))


def test_a_structured_operand_is_expanded_once(calls, both, monkeypatch):
    n = 4
    T_ = np.triu(int_dense((n, n), 23) + np.eye(n))
    S = T_ + T_.T - np.diag(np.diag(T_))
    expansions = []

    def symmetric_to_general(indptr, indices, values, uplo, value_dtype=None):
        assert uplo == "U"
        expansions.append(indptr)
        p, j, x = dense_to_csr(S)
        return dict(indptr=p, indices=j, values=x)
    monkeypatch.setattr(G, "csr_symmetric_to_general", symmetric_to_general)
    Sy = mx.dsRMatrix(*dense_to_csr(T_), (n, n), uplo="U")
    out = mx.crossprod(Sy)
    assert len(expansions) == 1 and len(calls) == 1 and calls[0][4:] == (True, "U")
    assert type(out) is dsRMatrix and np.array_equal(upper_dense(out), np.triu(S.T @ S))
    Tr = mx.dtRMatrix(*dense_to_csr(T_), (n, n), uplo="U", diag="N")
    out = mx.tcrossprod(Tr)                                              # diag "N": a relabel, no expansion
    assert len(expansions) == 1 and np.array_equal(upper_dense(out), np.triu(T_ @ T_.T))


def test_an_unsorted_operand_is_sorted_in_a_copy_for_both_forms(calls, both, monkeypatch):
    sorts = []

    def sort_inplace(p, j, x=None):
        sorts.append(j)
        for r in range(p.size - 1):
            o = np.argsort(j[p[r]:p[r + 1]], kind="stable")
            j[p[r]:p[r + 1]] = j[p[r]:p[r + 1]][o]
            if x is not None:
                x[p[r]:p[r + 1]] = x[p[r]:p[r + 1]][o]
    monkeypatch.setattr(G, "sort_sparse_indices_inplace", sort_inplace)
    D_ = np.ones((M_, K_)) * np.arange(1.0, K_ + 1)
    p, j, x = dense_to_csr(D_)
    X = mx.dgRMatrix(p, j[::-1].copy(), x[::-1].copy(), (M_, K_))      # every row descending
    before = X.j.copy()
    for k, signature in enumerate(("crossprod", "tcrossprod")):
        out = CALL[signature](X)
        assert len(sorts) == k + 1 and np.array_equal(X.j, before) and calls[-1][1] is not X.j   # X itself is not touched
        assert np.array_equal(calls[-1][1], j) and np.array_equal(calls[-1][2], x)
        assert np.array_equal(upper_dense(out), np.triu(DENSE[signature](D_)))


def test_validity_comes_before_the_export(calls, both):
    X = operand(int_dense((M_, K_), 24), "R", "x")
    bad = mx.dgRMatrix(X.p[:-1], X.j, X.x, (M_, K_))
    for call in CALL.values():
        with pytest.raises(mx.MatrixExtraError, match="Matrix is invalid"):
            call(bad)
    assert calls == []


def test_without_both_options_the_stand_in_is_never_reached(calls, monkeypatch):
    general = []
    monkeypatch.setattr(G, "csr_spgemm", lambda *a: general.append(a) or dict(
        indptr=np.zeros(a[3][1 if a[4] else 0] + 1, np.int32), indices=np.zeros(0, np.int32), values=np.zeros(0)))
    X = operand(int_dense((M_, K_), 25), "R", "x")
    assert not options.get("mxgpu.spgemm_route", False) and not options.get("mxgpu.gram_symmetric", False)
    for call in CALL.values():                                           # neither option: the usual stop
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types"):
            call(X)
    options["mxgpu.gram_symmetric"] = True                              # the new option alone changes nothing
    try:
        for call in CALL.values():
            with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types"):
                call(X)
    finally:
        options.pop("mxgpu.gram_symmetric", None)
    assert general == []
    options["mxgpu.spgemm_route"] = True                                # the route alone: the general matrix of before
    try:
        out = mx.crossprod(X)
        assert type(out) is mx.dgRMatrix and len(general) == 1
        options["mxgpu.gram_symmetric"] = True
        mx.crossprod(X, X)                                              # two arguments stay general under both options
        assert len(general) == 2
    finally:
        options.pop("mxgpu.spgemm_route", None)
        options.pop("mxgpu.gram_symmetric", None)
    assert calls == []


# ---- device.py on the recording fake ---------------------------------------------------------------------------------
def left():
    """4 x 3 with five entries"""
    return D.DeviceCSR(T.i32(0, 2, 2, 4, 5), T.i32(0, 2, 1, 2, 0), T.values("d", 5), 4, 3, 5)


def right(kind="l"):
    """3 x 4 with four entries, the middle row empty"""
    return T.csr(kind)


def run(operands, fn, script):
    return T.run_case(dict(operands=lambda: operands, run=fn, script=script))


def test_device_spgemm_with_a_mask_makes_the_two_tri_calls():
    A, B = left(), right()
    ws = T.workspace_bytes(4, 4)
    out = run(dict(A=A, B=B), lambda o: D.spgemm(o["A"], o["B"], uplo="L"),
              {"mxd_csr_rows_sorted": [[1]], "mxd_csr_spgemm_tri_count": [[9, 3]]})
    ops = [["A.indptr", 0], ["A.indices", 0]], [["B.indptr", 0], ["B.indices", 0]]
    assert out["calls"] == [
        {"fn": "mxd_csr_rows_sorted",
         "args": [3, ["B.indptr", 0], ["B.indices", 0], ["fresh#0", 0], ["cell", "int32"], "stream"]},
        {"fn": "mxd_csr_spgemm_workspace_bytes", "args": [4, 4]},
        {"fn": "mxd_csr_spgemm_tri_count",
         "args": [4, 3, 4, *ops[0], 5, *ops[1], 4, L, 1, ["fresh#2", 0], ["fresh#1", 0], ["cell", "int64"], ["cell", "int64"],
                  "stream"]},
        {"fn": "mxd_csr_spgemm_tri_fill",
         "args": [4, 3, 4, *ops[0], ["A.values", 0], F64, *ops[1], ["B.values", 0], _lib.MX_LGL, L, 1, ["fresh#2", 0],
                  ["fresh#3", 0], ["fresh#4", 0], ["fresh#1", 0], "stream"]}]
    assert out["allocations"] == [{"dtype": "torch.int32", "shape": [4]}, {"dtype": "torch.uint8", "shape": [ws]},
                                  {"dtype": "torch.int32", "shape": [5]}, {"dtype": "torch.int32", "shape": [3]},
                                  {"dtype": "torch.float64", "shape": [3]}]
    r = out["returns"]["DeviceCSR"]
    assert (r["m"], r["K"], r["nnz"]) == (4, 4, 3) and r["indptr"]["storage"] == ["fresh#2", 0]
    assert out["state"]["B"]["_sorted"] is True


def test_device_spgemm_without_a_mask_makes_the_calls_of_before():
    A, B = left(), right("d")
    out = run(dict(A=A, B=B), lambda o: D.spgemm(o["A"], o["B"]), {"mxd_csr_spgemm_count": [[7, 0]]})
    assert [c["fn"] for c in out["calls"]] == ["mxd_csr_spgemm_workspace_bytes", "mxd_csr_spgemm_count"]     # empty: no fill
    assert len(out["calls"][1]["args"]) == 14 and out["state"]["B"]["_sorted"] is None    # B's order is not asked for
    out = run(dict(A=left(), B=right("d")), lambda o: D.spgemm(o["A"], o["B"], None), {"mxd_csr_spgemm_count": [[7, 2]]})
    assert [c["fn"] for c in out["calls"]] == ["mxd_csr_spgemm_workspace_bytes", "mxd_csr_spgemm_count",
                                               "mxd_csr_spgemm_fill"]
    assert len(out["calls"][2]["args"]) == 16


def test_device_spgemm_refuses_a_bad_uplo_and_a_bad_shape_before_any_call():
    for uplo, message in (("u", "uplo must be 'U' or 'L'"), (0, "uplo must be 'U' or 'L'")):
        got = T.run_refusal(dict(operands=lambda: dict(A=left(), B=right()), run=lambda o: D.spgemm(o["A"], o["B"], uplo)))
        assert got == {"type": "ValueError", "message": message}
    got = T.run_refusal(dict(operands=lambda: dict(A=left(), B=right()), run=lambda o: D.spgemm(o["B"], o["B"], "U")))
    assert got == {"type": "ValueError", "message": "spgemm: A has 4 columns, B has 3 rows"}


def test_device_gram_goes_through_the_cached_order():
    """trans: spgemm(A^T, A, uplo), b_sorted from A's own rows; else spgemm(A, A^T, uplo), whose right-hand side is
    sorted by construction and not asked; a second call builds no second order"""
    script = {"mxd_csr_rows_sorted": [[0]], "mxd_csr_spgemm_tri_count": [[6, 2]]}

    def twice(trans):
        return lambda o: (D.gram(o["A"], trans=trans, uplo="U"), D.gram(o["A"], trans=trans, uplo="U"))
    out = run(dict(A=left()), twice(True), script)
    fns = [c["fn"] for c in out["calls"]]
    assert fns.count("mxd_csr_column_order") == 1 and out["state"]["A"] == {"_sorted": False, "_order_builds": 1}
    assert fns.count("mxd_csr_rows_sorted") == 1 and fns.count("mxd_csr_spgemm_tri_count") == 2
    count = [c for c in out["calls"] if c["fn"] == "mxd_csr_spgemm_tri_count"][0]["args"]
    assert count[:3] == [3, 4, 3] and count[6:8] == [["A.indptr", 0], ["A.indices", 0]] and count[9:11] == [U, 0]
    assert [r["DeviceCSR"]["m"] for r in out["returns"]] == [3, 3]
    out = run(dict(A=left()), twice(False), script)
    fns = [c["fn"] for c in out["calls"]]
    assert fns.count("mxd_csr_column_order") == 1 and "mxd_csr_rows_sorted" not in fns
    count = [c for c in out["calls"] if c["fn"] == "mxd_csr_spgemm_tri_count"][0]["args"]
    assert count[:3] == [4, 3, 4] and count[3:5] == [["A.indptr", 0], ["A.indices", 0]] and count[9:11] == [U, 1]
