"""The NA-keeping `CSR (op) dense vector` route, without a GPU: the new C-ABI entries (declared and, when the library
is built, exported), what multiply_csr_by_dvec_elemwise_internal (R/operators.R:996-1129) decides before and around the
export (which is monkeypatched here), and the numpy model of the route against hand-worked cases."""
import os
import warnings

import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G, operators
from dvec_na_model import (NA_BITS, NA_REAL, NAN, NAN_BITS, OPS, OTHER_NAN, compare, dirty_case, flags, make_csr,
                           make_vector, model)

INF = float("inf")
OPTION = "mxgpu.dvec_na_route"


@pytest.fixture
def route(monkeypatch):
    """the option set, and the export replaced by a recorder that answers with the model (on sorted input)"""
    calls = []

    def export(p, j, x, v, ncols, *fl):
        calls.append(dict(p=p, j=j, x=x, v=np.array(v), ncols=ncols, flags=fl))
        op = OPS[list(fl[:5]).index(True)]
        res = model(p, j, x, v, ncols, op, fl[5])
        return dict(indptr=res["indptr"], indices=res["indices"], values=res["values"])

    monkeypatch.setattr(G, "multiply_csr_by_dvec_with_NAs", export)
    monkeypatch.setitem(mx.options, OPTION, True)
    # sorting and validation stay on the host here
    def sort_inplace(p, j, x):
        for r in range(len(p) - 1):
            o = np.argsort(j[p[r]:p[r + 1]], kind="stable")
            j[p[r]:p[r + 1]] = j[p[r]:p[r + 1]][o]
            if x is not None:
                x[p[r]:p[r + 1]] = x[p[r]:p[r + 1]][o]
    monkeypatch.setattr(G, "sort_sparse_indices_inplace", sort_inplace)

    def coo_to_csr(i, j, values, nrow, ncol):                      # distinct cells only
        o = np.lexsort((j, i))
        p = np.zeros(nrow + 1, dtype=np.int32)
        p[1:] = np.cumsum(np.bincount(i, minlength=nrow))
        return dict(indptr=p, indices=np.asarray(j, dtype=np.int32)[o], values=np.asarray(values)[o])
    monkeypatch.setattr(G, "coo_to_csr", coo_to_csr)
    monkeypatch.setattr(operators, "check_valid_matrix", lambda e: None)
    import matrixextra_amd.matrices as M
    monkeypatch.setattr(M, "check_valid_matrix", lambda e: None)
    return calls


def _X():
    return mx.dgRMatrix([0, 2, 3, 3, 4], [2, 0, 1, 0], [2.0, 1.0, 3.0, 4.0], (4, 3), [list("abcd"), None])


def test_entry_points_declared_and_exported():
    wanted = {"mx_multiply_csr_by_dvec_with_NAs_begin", "mxd_csr_by_dvec_na_rows_workspace_bytes",
              "mxd_csr_by_dvec_na_rows_count", "mxd_csr_by_dvec_na_rows_fill", "mxd_dvec_na_special_workspace_bytes",
              "mxd_dvec_na_special", "mxd_dvec_na_cells_workspace_bytes", "mxd_dvec_na_cells_count",
              "mxd_dvec_na_cells_fill", "mxd_csr_join_disjoint"}
    header = open(_lib.HEADER_PATH).read()
    assert all(s + "(" in header for s in wanted)
    assert {s for s in wanted if s == s.lower()} <= set(_lib.declared_symbols())     # its pattern is lower case
    assert "multiply_csr_by_dvec_with_NAs, :2258-) is not provided" not in header
    assert "#define MXGPU_ABI_VERSION 1" in header
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, s) for s in wanted)
        assert lib.mxd_csr_by_dvec_na_rows_workspace_bytes(1000) >= 4 * 1000
        assert lib.mxd_dvec_na_special_workspace_bytes(1000) >= 3 * 4 * 1000
        assert lib.mxd_dvec_na_cells_workspace_bytes(1000) >= 2 * 4 * 1000
    assert callable(G.multiply_csr_by_dvec_with_NAs)
    import rshim_registry
    rshim_registry.assert_shim_and_overlay_carry("multiply_csr_by_dvec_with_NAs", 11)


def test_option_off_raises_as_before(monkeypatch):
    monkeypatch.setattr(G, "multiply_csr_by_dvec_with_NAs", lambda *a: pytest.fail("the export was reached"))
    monkeypatch.setattr(operators, "check_valid_matrix", lambda e: None)
    assert not mx.options.get(OPTION, False)
    X = _X()
    for op, v in (("*", [1.0, np.nan]), ("/", [0.0, 1.0]), ("*", [INF, 1.0]), ("^", [-1.0, 2.0]), ("%%", [0.0, 2.0])):
        with pytest.raises(mx.MatrixExtraError, match=r"R/operators.R:981-1131\), which is not on the accelerated path"):
            operators.csr_op_vector(X, np.array(v), op)
    monkeypatch.setitem(mx.options, OPTION, False)
    with pytest.raises(mx.MatrixExtraError, match="981-1131"):
        operators.csr_op_vector(X, np.array([0.0, 1.0]), "/")


def test_route_call_order_class_and_dimnames(route):
    X = _X()                                                        # row 0 is unsorted
    j0, x0 = X.j.copy(), X.x.copy()
    out = operators.csr_op_vector(X, np.array([0.0, 4.0]), "/")
    assert len(route) == 1
    call = route[0]
    assert list(call["j"]) == [0, 2, 1, 0] and list(call["x"]) == [1.0, 2.0, 3.0, 4.0]       # sorted before the call
    assert call["ncols"] == 3 and call["flags"] == (False, False, True, False, False, True)
    assert list(X.j) == list(j0) and list(X.x) == list(x0) and call["j"] is not X.j          # X itself untouched
    assert type(out) is mx.dgRMatrix and tuple(out.Dim) == (4, 3) and out.Dimnames[0] == list("abcd")
    exp = model(call["p"], call["j"], call["x"], [0.0, 4.0], 3, "/")
    assert list(out.p) == list(exp["indptr"]) and list(out.j) == list(exp["indices"])
    assert list(out.p) == [0, 3, 4, 7, 8]


def test_route_inplace_sort_sorts_the_operand(route, monkeypatch):
    monkeypatch.setitem(mx.options, "MatrixExtra.inplace_sort", True)
    X = _X()
    operators.csr_op_vector(X, np.array([0.0, 4.0]), "/")
    assert route[0]["j"] is X.j and list(X.j) == [0, 2, 1, 0]       # a dgRMatrix is sorted where it is
    L = mx.lgRMatrix([0, 2, 2], [1, 0], [1, 1], (2, 2))
    operators.csr_op_vector(L, np.array([np.nan, 1.0]), "*")
    assert list(L.j) == [1, 0]                                      # any other class is copied first (:1013-1014)


def test_route_coo_operand_and_warning(route):
    T = mx.dgTMatrix([1, 0, 0], [1, 2, 0], [3.0, 2.0, 1.0], (3, 3), [None, list("xyz")])
    i0 = T.i.copy()
    with pytest.warns(UserWarning, match="Number of elements in vector is not a multiple of matrix dimension."):
        out = operators.csr_op_vector(T, np.array([1.0, np.nan]), "*")
    assert type(out) is mx.dgRMatrix and tuple(out.Dim) == (3, 3) and out.Dimnames[1] == list("xyz")
    assert list(route[0]["p"]) == [0, 2, 3, 3] and list(route[0]["j"]) == [0, 2, 1]          # a CSR reached the export
    assert list(T.i) == list(i0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        operators.csr_op_vector(T, np.array([1.0, np.nan, 2.0]), "*")                       # 3 divides 3: no warning
    assert route[-1]["flags"] == (True, False, False, False, False, True)
    operators.csr_op_vector(T, np.array([1.0, INF, 2.0]), "*", X_is_LHS=False)
    assert route[-1]["flags"][5] is False


def test_route_refusals(route):
    X = _X()
    n = len(route)
    for v in ([np.nan, np.nan], [NA_REAL] * 4):
        with pytest.raises(mx.MatrixExtraError, match=r"R/operators.R:998-1006\), which is not on the accelerated path"):
            operators.csr_op_vector(X, np.array(v), "*")
    with pytest.raises(mx.MatrixExtraError, match="998-1006"):
        operators.csr_op_vector(X, np.array([np.nan]), "/")
    with pytest.raises(mx.MatrixExtraError, match="1052-1056"):
        operators.csr_op_vector(X, np.array([INF]), "*")
    for op in ("/", "%%", "%/%"):
        with pytest.warns(UserWarning, match="division by zero"), pytest.raises(mx.MatrixExtraError, match="1063-1069"):
            operators.csr_op_vector(X, np.array([0.0]), op)
    for e in (0.0, -2.0):
        with pytest.raises(mx.MatrixExtraError, match="1085-1089"):
            operators.csr_op_vector(X, np.array([e]), "^")
    for op in ("^", "/", "%%", "%/%"):
        with pytest.raises(mx.MatrixExtraError, match="973-978"):
            operators.csr_op_vector(X, np.array([0.0, 1.0]), op, X_is_LHS=False)
    assert len(route) == n                                          # none of them reached the export
    # without anything special in the vector the values-only route is taken, option or not
    seen = []
    import matrixextra_amd.exports as E
    orig = E.multiply_csr_by_dvec_no_NAs_numeric
    try:
        E.multiply_csr_by_dvec_no_NAs_numeric = lambda *a: seen.append(a) or np.zeros(4)
        operators.csr_op_vector(X, np.array([1.0, 2.0]), "*")
    finally:
        E.multiply_csr_by_dvec_no_NAs_numeric = orig
    assert len(seen) == 1 and len(route) == n


def _bits(a):
    return [int(b) for b in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)]


HAND_P, HAND_J, HAND_X = [0, 1, 1], [1], [2.0]
HAND = [
    ("/", [0.0, 4.0], [0, 3, 3], [0, 1, 2], [NAN, INF, NAN]),
    ("*", [NA_REAL, INF], [0, 3, 6], [0, 1, 2, 0, 1, 2], [NA_REAL] * 3 + [NAN] * 3),
    ("*", [1.0, NA_REAL, 5.0], [0, 2, 3], [1, 2, 0], [10.0, NAN, NAN]),
    ("*", [1.0, OTHER_NAN, 5.0], [0, 2, 3], [1, 2, 0], [10.0, NA_REAL, NA_REAL]),
    ("^", [0.0, 2.0, -1.0], [0, 2, 4], [0, 1, 1, 2], [1.0, 0.5, 1.0, INF]),
]


@pytest.mark.parametrize("op,v,p,j,x", HAND, ids=[f"{h[0]}-{len(h[1])}-{k}" for k, h in enumerate(HAND)])
def test_model_hand_worked(op, v, p, j, x):
    res = model(HAND_P, HAND_J, HAND_X, v, 3, op)
    assert list(res["indptr"]) == p and list(res["indices"]) == j
    assert _bits(res["values"]) == _bits(x)
    assert NA_BITS != NAN_BITS


def test_model_alias_and_refusal():
    p, j, x = np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.arange(1.0, 5.0)
    res = model(p, j, x, [1.0, NA_REAL, 2.0], 2, "*")              # every cell stored: nothing to add
    assert res["alias"] and res["indptr"] is p and res["indices"] is j and res["candidates"] == 1
    with pytest.raises(ValueError, match="Internal error"):
        model(p, j, x, [0.0, 1.0, 1.0], 2, "/", X_is_LHS=False)


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("op", ["*", "/"])
def test_dirty_case_stays_under_the_cap(op, flat):
    """the dedicated NaN / Inf / 0 case of the GPU tests: the exemption is used, and covers at most 5 %"""
    p, j, x, v, ncols = dirty_case(op, flat)
    exp = model(p, j, x, v, ncols, op)
    share = compare(dict(indptr=exp["indptr"], indices=exp["indices"], values=exp["values"]), exp, op)
    assert 0 < share <= 0.05
    assert exp["fill"].any() and not exp["alias"]


def test_main_generators_need_no_exemption():
    for op in OPS:
        p, j, x = make_csr(30, 17, 0.3, 3, empty_rows=(0,), full_rows=(4,), positive=op == "^")
        for L in (10, 11):
            v = make_vector(L, op, 9, at=(0, L - 1))
            exp = model(p, j, x, v, 17, op)
            assert not exp["exempt"].any() and exp["fill"].any(), (op, L)
    assert flags("%%") == (False, False, False, True, False)
