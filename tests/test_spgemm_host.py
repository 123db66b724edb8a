"""The sparse x sparse products before a device call: include/mxgpu_spgemm.h as the binding reads it, the failures on bad
arguments, and what the `%*%` / crossprod / tcrossprod dispatch of matmul.py decides under options["mxgpu.spgemm_route"]:
the flags and the operand order of the one export call, the class, Dim and Dimnames of the result, for every signature
and layout, the one-argument forms and structured operands.  exports.csr_spgemm is replaced by a numpy stand-in, so no
GPU is needed.  Without the option every call stops as before and the stand-in is never reached."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import matrixextra_amd as mx
from conftest import csr_to_dense
from matrixextra_amd import _lib, exports as G, matmul
from matrixextra_amd.matrices import options

NEW = ["mx_csr_spgemm_begin", "mxd_csr_spgemm_count", "mxd_csr_spgemm_fill", "mxd_csr_spgemm_limits",
       "mxd_csr_spgemm_workspace_bytes"]
P, I, I64 = C.c_void_p, C.c_int, C.c_int64
F64, F32, LGL, NONE = _lib.MX_F64, _lib.MX_F32, _lib.MX_LGL, _lib.MX_NONE


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_spgemm_header_parses_and_is_bound_on_the_same_library():
    with open(_lib.SPGEMM_HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert sorted(h.functions) == NEW == sorted(_lib.SPGEMM_HEADER.functions)
    assert h.constants == {} and h.structs == {}
    assert h.functions["mxd_csr_spgemm_workspace_bytes"] == (C.c_size_t, (I, I))
    assert h.functions["mxd_csr_spgemm_limits"] == (I, (I, I, P, P, P))
    assert h.functions["mxd_csr_spgemm_count"] == (I, (I, I, I, P, P, I64, P, P, I64, P, P, P, P, P))
    assert h.functions["mxd_csr_spgemm_fill"] == (I, (I, I, I, P, P, P, I, P, P, P, I, P, P, P, P, P))
    assert h.functions["mx_csr_spgemm_begin"] == (I, (P, I, I, P, P, I, I, P, I, I, P, P, I, I, P, P))
    lib = _lib.load()
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)                                         # exported by libmxgpu.so
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name


def test_the_other_headers_keep_their_prototypes():
    assert not set(NEW) & set(_lib.declared_symbols()) and not set(NEW) & set(_lib.HEADER.functions)
    others = set(_lib.REDUCE_HEADER.functions) | set(_lib.SYM_HEADER.functions) | set(_lib.TPROD_HEADER.functions)
    assert not set(NEW) & others
    assert sorted(_lib.TPROD_HEADER.functions) == ["mx_csr_tmatmul_dense", "mx_csr_tmatvec", "mxd_csr_transpose_by_order",
                                                   "mxd_segment_dot"]
    with open(_lib.HEADER_PATH, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "272d0958dbaeeea098083be2d23248951d00c8726dc60aa6e5f6792e8f5b88b3"


def test_every_device_prototype_states_its_synchronisation():
    with open(_lib.SPGEMM_HEADER_PATH) as f:
        text = f.read()
    for name, waits in (("mxd_csr_spgemm_limits", False), ("mxd_csr_spgemm_count", True), ("mxd_csr_spgemm_fill", False)):
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == waits and ("no synchronisation" in comment) == (not waits), name


def test_the_limits_and_the_workspace_size():
    lib = _lib.load()
    sizes = {}
    for m, n in [(0, 0), (1, 1), (24, 1024), (24, 1027), (200000, 100000), (5, 2 ** 31 - 1)]:
        g, l, d = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.mxd_csr_spgemm_limits(m, n, C.byref(g), C.byref(l), C.byref(d)) == 0
        assert 0 < g.value < l.value and d.value >= 1
        assert 2 * l.value * 12 <= 64 * 1024                            # the workgroup's table: at most 64 KiB of LDS
        sizes[m, n] = lib.mxd_csr_spgemm_workspace_bytes(m, n)
        dense = d.value * (8 * n + 4 * ((n + 31) // 32)) if n > l.value else 0     # no row reaches the dense bin below that
        assert sizes[m, n] >= dense + 4 * 4 * m
        assert n > l.value or sizes[m, n] <= 64 + 48 * (m + 4) + 1024
    assert lib.mxd_csr_spgemm_limits(3, 3, None, None, None) == 0       # any of the three may be null
    assert sizes[200000, 100000] < 2 ** 29                              # the accumulators stay under their cap


def test_calls_fail_loudly_on_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.mx_last_error().decode()                          # noqa: E731
    assert lib.mxd_csr_spgemm_limits(-1, 3, None, None, None) != 0 and "negative dimension" in err()
    assert lib.mxd_csr_spgemm_count(-1, 1, 1, None, None, 0, None, None, 0, None, None, None, None, None) != 0
    assert "negative dimension" in err()
    assert lib.mxd_csr_spgemm_count(1, 1, 1, None, None, -1, None, None, 0, None, None, None, None, None) != 0
    assert "bad size" in err()
    assert lib.mxd_csr_spgemm_count(1, 1, 1, None, None, 0, None, None, 0, None, None, None, None, None) != 0
    assert "null pointer" in err()
    assert lib.mxd_csr_spgemm_fill(1, 1, -1, None, None, None, F64, None, None, None, F64, None, None, None, None, None) != 0
    assert "negative dimension" in err()
    for bad in ((F32, F64), (F64, _lib.MX_I32), (7, NONE)):
        assert lib.mxd_csr_spgemm_fill(1, 1, 1, None, None, None, bad[0], None, None, None, bad[1], None, None, None, None,
                                       None) != 0
        assert "unsupported value dtype" in err()
    assert lib.mxd_csr_spgemm_fill(1, 1, 1, None, None, None, F64, None, None, None, LGL, None, None, None, None, None) != 0
    assert "null pointer" in err()
    assert lib.mxd_csr_spgemm_fill(0, 1, 1, None, None, None, NONE, None, None, None, NONE, None, None, None, None, None) == 0
    p = np.zeros(3, np.int32)
    res, info = C.c_void_p(), _lib.ResultInfo()
    begin = lambda *a: lib.mx_csr_spgemm_begin(*a, C.byref(res), C.byref(info))     # noqa: E731
    assert lib.mx_csr_spgemm_begin(_lib.ptr(p), 2, 2, None, None, F64, 0, _lib.ptr(p), 2, 2, None, None, F64, 0, None,
                                   None) != 0 and "null pointer" in err()
    assert begin(None, 2, 2, None, None, F64, 0, _lib.ptr(p), 2, 2, None, None, F64, 0) != 0 and "null pointer" in err()
    assert begin(_lib.ptr(p), 2, -2, None, None, F64, 0, _lib.ptr(p), 2, 2, None, None, F64, 0) != 0
    assert "negative dimension" in err()
    assert begin(_lib.ptr(p), 2, 2, None, None, F32, 0, _lib.ptr(p), 2, 2, None, None, F64, 0) != 0
    assert "unsupported value dtype" in err()
    bad_p = np.array([0, 1, -1], np.int32)
    assert begin(_lib.ptr(p), 2, 2, None, None, F64, 0, _lib.ptr(bad_p), 2, 2, None, None, F64, 0) != 0
    assert "bad index pointer" in err()
    one = np.array([0, 1, 1], np.int32)
    assert begin(_lib.ptr(one), 2, 2, None, None, F64, 0, _lib.ptr(p), 2, 2, None, None, F64, 0) != 0 and "null pointer" in err()
    # the inner dimensions are checked after the transposes: 2 x 3 times 2 x 3 fits only with one side transposed
    for ta, tb, ok in ((0, 0, False), (1, 1, False)):
        assert begin(_lib.ptr(p), 2, 3, None, None, NONE, ta, _lib.ptr(p), 2, 3, None, None, NONE, tb) != 0
        assert "inner dimensions differ" in err()
    with pytest.raises(ValueError, match="indptr and dims disagree"):
        G.csr_spgemm(p, np.zeros(0, np.int32), None, (3, 2), False, p, np.zeros(0, np.int32), None, (2, 2), False)


# ---- the mirror --------------------------------------------------------------------------------------------------------
M_, K_, N_ = 4, 5, 3
SHAPES = {"matmult": ((M_, K_), (K_, N_)), "crossprod": ((K_, M_), (K_, N_)), "tcrossprod": ((M_, K_), (N_, K_))}
CALL = {"matmult": lambda x, y: x @ y, "crossprod": mx.crossprod, "tcrossprod": mx.tcrossprod}
DENSE = {"matmult": lambda X, Y: X @ Y, "crossprod": lambda X, Y: X.T @ Y, "tcrossprod": lambda X, Y: X @ Y.T}
# (trans_a, trans_b, operands swapped) of the export call, written out: a CSC operand's arrays are the CSR of its transpose
FLAGS = {("matmult", "R", "R"): (False, False, False), ("matmult", "R", "C"): (False, True, False),
         ("matmult", "C", "R"): (True, False, False), ("matmult", "C", "C"): (False, False, True),
         ("crossprod", "R", "R"): (True, False, False), ("crossprod", "R", "C"): (True, True, False),
         ("crossprod", "C", "R"): (False, False, False), ("crossprod", "C", "C"): (False, True, True),
         ("tcrossprod", "R", "R"): (False, True, False), ("tcrossprod", "R", "C"): (False, False, False),
         ("tcrossprod", "C", "R"): (True, True, False), ("tcrossprod", "C", "C"): (True, False, True)}


def dense_to_csr(D, keep=None):
    keep = (D != 0) if keep is None else keep
    p = np.zeros(D.shape[0] + 1, dtype=np.int32)
    p[1:] = np.cumsum(keep.sum(axis=1))
    r, c = np.nonzero(keep)
    return p, c.astype(np.int32), D[r, c]


def int_dense(shape, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.5, rng.integers(1, 5, size=shape), 0).astype(np.float64)


def operand(D, layout, tag):
    dn = [["%sr%d" % (tag, r) for r in range(D.shape[0])], ["%sc%d" % (tag, c) for c in range(D.shape[1])]]
    if layout == "R":
        return mx.dgRMatrix(*dense_to_csr(D), D.shape, dn)
    return mx.dgCMatrix(*dense_to_csr(D.T), D.shape, dn)


@pytest.fixture
def calls(monkeypatch):
    """exports.csr_spgemm records its arguments and answers in numpy; the sortedness check answers in numpy too"""
    seen = []

    def csr_spgemm(p1, j1, x1, dims1, trans_a, p2, j2, x2, dims2, trans_b):
        seen.append((p1, j1, x1, tuple(dims1), trans_a, p2, j2, x2, tuple(dims2), trans_b))
        ops = []
        for p, j, x, dims, t in ((p1, j1, x1, dims1, trans_a), (p2, j2, x2, dims2, trans_b)):
            assert p.size == dims[0] + 1
            V = csr_to_dense(p, j, np.ones(j.size) if x is None else np.where(x == mx.NA_INTEGER, np.nan, x), dims[1])
            S = csr_to_dense(p, j, np.ones(j.size), dims[1])
            ops.append((V.T, S.T) if t else (V, S))
        assert ops[0][0].shape[1] == ops[1][0].shape[0]
        with np.errstate(invalid="ignore"):
            out = np.nan_to_num(ops[0][0]) @ np.nan_to_num(ops[1][0])
        p, j, x = dense_to_csr(out, keep=(ops[0][1] @ ops[1][1]) != 0)
        return dict(indptr=p, indices=j, values=x)

    monkeypatch.setattr(G, "csr_spgemm", csr_spgemm)
    monkeypatch.setattr(G, "check_indices_are_sorted",
                        lambda p, j: all(np.all(np.diff(j[p[r]:p[r + 1]]) > 0) for r in range(p.size - 1)))
    return seen


@pytest.fixture
def route():
    options["mxgpu.spgemm_route"] = True
    yield
    options.pop("mxgpu.spgemm_route", None)


@pytest.mark.parametrize("signature,lx,ly", sorted(FLAGS))
def test_every_signature_and_layout(calls, route, signature, lx, ly):
    (sx, sy) = SHAPES[signature]
    DX, DY = int_dense(sx, 1), int_dense(sy, 2)
    X, Y = operand(DX, lx, "x"), operand(DY, ly, "y")
    out = CALL[signature](X, Y)
    (p1, j1, x1, d1, ta, p2, j2, x2, d2, tb), = calls
    want_ta, want_tb, swap = FLAGS[signature, lx, ly]
    assert (ta, tb) == (want_ta, want_tb) == matmul.spgemm_flags(signature, lx, ly)[:2]
    first, second = (Y, X) if swap else (X, Y)
    idx = lambda o: o.j if isinstance(o, mx.RsparseMatrix) else o.i     # noqa: E731
    raw = lambda o: o.Dim if isinstance(o, mx.RsparseMatrix) else o.Dim[::-1]    # noqa: E731
    assert p1 is first.p and j1 is idx(first) and x1 is first.x and d1 == raw(first)     # the arrays as they are
    assert p2 is second.p and j2 is idx(second) and x2 is second.x and d2 == raw(second)
    want = DENSE[signature](DX, DY)
    assert type(out) is (mx.dgCMatrix if swap else mx.dgRMatrix) and swap == (lx == ly == "C")
    assert out.Dim == want.shape == (M_, N_)
    got = csr_to_dense(out.p, out.i, out.x, M_).T if swap else csr_to_dense(out.p, out.j, out.x, N_)
    assert np.array_equal(got, want)
    rn = X.Dimnames[1] if signature == "crossprod" else X.Dimnames[0]
    cn = Y.Dimnames[0] if signature == "tcrossprod" else Y.Dimnames[1]
    assert out.Dimnames == [rn, cn]


def test_logical_and_pattern_operands_keep_their_values_for_the_export(calls, route):
    D = int_dense((M_, K_), 3)
    p, j, _ = dense_to_csr(D)
    xl = np.where(np.arange(j.size) % 3 == 0, mx.NA_INTEGER, 1).astype(np.int32)
    L, N = mx.lgRMatrix(p, j, xl, (M_, K_)), mx.ngRMatrix(p, j, None, (M_, K_))
    Y = operand(int_dense((K_, N_), 4), "R", "y")
    out = L @ Y
    assert calls[-1][2] is L.x and calls[-1][2].dtype == np.int32 and type(out) is mx.dgRMatrix and out.x.dtype == np.float64
    out = mx.tcrossprod(N, N)
    assert calls[-1][2] is None and calls[-1][7] is None and calls[-1][4:10:5] == (False, True)
    assert np.array_equal(csr_to_dense(out.p, out.j, out.x, M_), (D != 0).astype(float) @ (D != 0).astype(float).T)


def test_the_one_argument_forms(calls, route):
    D = int_dense((M_, K_), 5)
    X, Cx = operand(D, "R", "x"), operand(D, "C", "x")
    out = mx.crossprod(X)
    assert calls[-1][0] is X.p and calls[-1][5] is X.p and (calls[-1][4], calls[-1][9]) == (True, False)
    assert type(out) is mx.dgRMatrix and out.Dim == (K_, K_) and out.Dimnames == [X.Dimnames[1], X.Dimnames[1]]
    assert np.array_equal(csr_to_dense(out.p, out.j, out.x, K_), D.T @ D)             # the general matrix, both triangles
    out = mx.tcrossprod(X)
    assert (calls[-1][4], calls[-1][9]) == (False, True) and out.Dim == (M_, M_)
    assert np.array_equal(csr_to_dense(out.p, out.j, out.x, M_), D @ D.T) and out.Dimnames == [X.Dimnames[0]] * 2
    out = mx.crossprod(Cx)
    assert type(out) is mx.dgCMatrix and out.Dim == (K_, K_) and np.array_equal(csr_to_dense(out.p, out.i, out.x, K_), D.T @ D)
    out = mx.tcrossprod(Cx)
    assert type(out) is mx.dgCMatrix and out.Dim == (M_, M_) and np.array_equal(csr_to_dense(out.p, out.i, out.x, M_), D @ D.T)
    assert len(calls) == 4


def test_an_unsorted_right_hand_operand_is_sorted_in_a_copy(calls, route, monkeypatch):
    sorts = []

    def sort_inplace(p, j, x=None):
        sorts.append(j)
        for r in range(p.size - 1):
            o = np.argsort(j[p[r]:p[r + 1]], kind="stable")
            j[p[r]:p[r + 1]] = j[p[r]:p[r + 1]][o]
            if x is not None:
                x[p[r]:p[r + 1]] = x[p[r]:p[r + 1]][o]
    monkeypatch.setattr(G, "sort_sparse_indices_inplace", sort_inplace)
    DX, DY = int_dense((M_, K_), 6), np.ones((K_, N_)) * np.arange(1.0, N_ + 1)
    p, j, x = dense_to_csr(DY)
    Y = mx.dgRMatrix(p, j[::-1].copy(), x[::-1].copy(), (K_, N_))      # every row descending
    X = operand(DX, "R", "x")
    before = Y.j.copy()
    out = X @ Y
    assert len(sorts) == 1 and np.array_equal(Y.j, before) and calls[-1][6] is not Y.j      # Y itself is not touched
    assert np.array_equal(calls[-1][6], j) and np.array_equal(csr_to_dense(out.p, out.j, out.x, N_), DX @ DY)
    Xu = mx.dgRMatrix(X.p, X.j[::-1].copy(), X.x[::-1].copy(), (M_, K_))
    Xu @ operand(DY, "R", "y")                                         # the left-hand operand may stay unsorted
    assert len(sorts) == 1 and calls[-1][1] is Xu.j


def test_structured_operands_go_through_their_general_class(calls, route, monkeypatch):
    n = 4
    T = np.triu(int_dense((n, n), 7) + np.eye(n))
    S = T + T.T - np.diag(np.diag(T))

    expansions = []

    def symmetric_to_general(indptr, indices, values, uplo, value_dtype=None):
        assert uplo == "U"
        expansions.append(indptr)
        p, j, x = dense_to_csr(S)
        return dict(indptr=p, indices=j, values=x)
    monkeypatch.setattr(G, "csr_symmetric_to_general", symmetric_to_general)
    monkeypatch.setattr(G, "csr_triangle_check", lambda p, j, uplo, strict=False: 0)
    Sy = mx.dsRMatrix(*dense_to_csr(T), (n, n), uplo="U")
    Tr = mx.dtRMatrix(*dense_to_csr(T), (n, n), uplo="U", diag="N")
    Y = operand(int_dense((n, N_), 8), "R", "y")
    out = Sy @ Y
    assert type(out) is mx.dgRMatrix and np.array_equal(csr_to_dense(out.p, out.j, out.x, N_), S @ Y.toarray())
    out = mx.crossprod(Tr, Sy)
    assert (calls[-1][4], calls[-1][9]) == (True, False) and np.array_equal(csr_to_dense(out.p, out.j, out.x, n), T.T @ S)
    out = mx.tcrossprod(Tr)
    assert np.array_equal(csr_to_dense(out.p, out.j, out.x, n), T @ T.T)
    del expansions[:]
    out = mx.crossprod(Sy)                                              # one expansion serves both sides
    assert len(expansions) == 1 and calls[-1][0] is calls[-1][5] and calls[-1][2] is calls[-1][7]
    assert np.array_equal(csr_to_dense(out.p, out.j, out.x, n), S.T @ S)


def test_dimension_and_validity_errors_come_before_the_export(calls, route):
    X, Y = operand(int_dense((M_, K_), 9), "R", "x"), operand(int_dense((M_, N_), 10), "C", "y")
    for call in (lambda: X @ Y, lambda: mx.tcrossprod(X, Y), lambda: mx.crossprod(X, operand(int_dense((K_, N_), 11), "R", "y"))):
        with pytest.raises(mx.MatrixExtraError, match="Matrix dimensions do not match."):
            call()
    bad = mx.dgRMatrix(X.p[:-1], X.j, X.x, (M_, K_))
    with pytest.raises(mx.MatrixExtraError, match="Matrix is invalid"):
        mx.tcrossprod(bad, X)
    assert calls == []


# what each call of two sparse matrices ends in without the option, as it did before the route existed: the dispatch
# falls into a branch written for a dense operand, which stops with its own message or fails on the operand's shape
UNSUPPORTED, MISMATCH, NO_SHAPE = "Unsupported operand types for %s", "Matrix dimensions do not match.", "tuple index out of range"
BEFORE = {("R", "R", "matmult"): (IndexError, NO_SHAPE), ("R", "C", "matmult"): (IndexError, NO_SHAPE),
          ("C", "R", "matmult"): (mx.MatrixExtraError, UNSUPPORTED % "%\\*%"), ("C", "C", "matmult"): (mx.MatrixExtraError, MISMATCH),
          ("R", "R", "crossprod"): (mx.MatrixExtraError, UNSUPPORTED % "crossprod"), ("R", "C", "crossprod"): (IndexError, NO_SHAPE),
          ("C", "R", "crossprod"): (mx.MatrixExtraError, UNSUPPORTED % "crossprod"), ("C", "C", "crossprod"): (IndexError, NO_SHAPE),
          ("R", "R", "tcrossprod"): (mx.MatrixExtraError, MISMATCH), ("R", "C", "tcrossprod"): (mx.MatrixExtraError, MISMATCH),
          ("C", "R", "tcrossprod"): (mx.MatrixExtraError, MISMATCH),
          ("C", "C", "tcrossprod"): (mx.MatrixExtraError, UNSUPPORTED % "tcrossprod")}


def test_without_the_option_every_call_stops_as_before(calls):
    assert not options.get("mxgpu.spgemm_route", False)
    D = int_dense((M_, M_), 12)
    assert sorted(BEFORE) == sorted(itertools.product("RC", "RC", CALL))
    for (lx, ly, signature), (error, message) in BEFORE.items():
        X, Y = operand(D, lx, "x"), operand(D, ly, "y")
        with pytest.raises(error, match=message) as caught:
            CALL[signature](X, Y)
        assert type(caught.value) is error, (lx, ly, signature)
    X, Cx = operand(D, "R", "x"), operand(D, "C", "x")
    for o in (X, Cx):
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for crossprod"):
            mx.crossprod(o)
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for tcrossprod"):
            mx.tcrossprod(o)
    with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for crossprod"):
        mx.crossprod(X, X)
    with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for %\\*%"):
        matmul.matmul(Cx, X)
    options["mxgpu.spgemm_route"] = True                                # one-argument forms of anything else still stop
    try:
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for crossprod"):
            mx.crossprod(np.ones((3, 3)))
    finally:
        options.pop("mxgpu.spgemm_route", None)
    assert calls == []
