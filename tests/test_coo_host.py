"""COO (TsparseMatrix) surface checks that need no GPU: the classes and their slots, t() as a shallow swap,
check_valid_matrix, as_coo_matrix's flag rules, operator dispatch to the COO paths, and the new C-ABI entries
(declared, exported, failing loudly without a device)."""
import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G, operators


def _coo(cls=mx.dgTMatrix):
    i = np.array([2, 0, 1, 0], np.int32)
    j = np.array([1, 3, 0, 3], np.int32)
    x = None if cls is mx.ngTMatrix else (np.array([1.5, 2.0, -1.0, 0.5]) if cls is mx.dgTMatrix
                                          else np.array([1, 0, -2147483648, 1], np.int32))
    return cls(i, j, x, (3, 4), [["a", "b", "c"], ["w", "x", "y", "z"]])


def test_coo_entry_points_declared_and_exported():
    names = set(_lib.declared_symbols())
    wanted = {"mx_coo_to_csr_begin", "mx_csr_to_coo", "mx_multiply_csr_by_coo_begin",
              "mx_multiply_coo_by_dense_ignore_NAs_numeric", "mx_multiply_coo_by_dense_ignore_NAs_logical",
              "mxd_coo_to_csr", "mxd_coo_to_csr_workspace_bytes", "mxd_csr_to_coo", "mxd_csr_by_coo_count",
              "mxd_csr_by_coo_fill", "mxd_csr_by_coo_workspace_bytes", "mxd_coo_by_dvec"}
    assert {w for w in wanted if w == w.lower()} <= names     # the header scan matches lower-case names only
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in wanted)


def test_coo_workspace_sizes():
    lib = _lib.load()
    nnz = 1 << 20
    assert lib.mxd_coo_to_csr_workspace_bytes(nnz, 1000) > lib.mxd_csr_transpose_workspace_bytes(nnz)
    assert lib.mxd_coo_to_csr_workspace_bytes(nnz, 1 << 20) >= lib.mxd_coo_to_csr_workspace_bytes(nnz, 1000) + 4 * 1000
    assert lib.mxd_csr_by_coo_workspace_bytes(nnz) >= 8 * nnz


@pytest.mark.parametrize("cls, dtype", [(mx.dgTMatrix, np.float64), (mx.lgTMatrix, np.int32), (mx.ngTMatrix, None)])
def test_classes_and_slots(cls, dtype):
    T = _coo(cls)
    assert isinstance(T, mx.TsparseMatrix) and T.r_class == cls.__name__
    assert T.i.dtype == np.int32 and T.j.dtype == np.int32
    assert (T.x is None) if dtype is None else (T.x.dtype == dtype)
    assert T.Dim == (3, 4) and T.nrow() == 3 and T.ncol() == 4
    assert T.Dimnames == [["a", "b", "c"], ["w", "x", "y", "z"]]
    c = T.copy()
    assert type(c) is cls and c.i is not T.i and np.array_equal(c.i, T.i)


def test_toarray_combines_duplicates():
    assert _coo().toarray()[0, 3] == 2.5
    lg = _coo(mx.lgTMatrix).toarray()
    assert lg[0, 3] == 1.0 and np.isnan(lg[1, 0]) and lg[2, 1] == 1.0
    assert _coo(mx.ngTMatrix).toarray().sum() == 3.0


def test_t_is_a_shallow_swap():
    T = _coo()
    U = T.t()
    assert type(U) is mx.dgTMatrix
    assert U.i is T.j and U.j is T.i and U.x is T.x
    assert U.Dim == (4, 3) and U.Dimnames == [["w", "x", "y", "z"], ["a", "b", "c"]]
    assert mx.t_shallow(T).i is T.j


def test_check_valid_matrix_messages():
    T = _coo()
    mx.check_valid_matrix(T)
    bad = _coo()
    bad.j = bad.j[:3]
    with pytest.raises(mx.MatrixExtraError, match="row and column indices have different length"):
        mx.check_valid_matrix(bad)
    bad = _coo()
    bad.x = bad.x[:2]
    with pytest.raises(mx.MatrixExtraError, match="values and indices have different number of entries"):
        mx.check_valid_matrix(bad)
    bad = _coo()
    bad.Dimnames = [["a"], None]
    with pytest.raises(mx.MatrixExtraError, match="Row names"):
        mx.check_valid_matrix(bad)


def test_as_coo_flag_rules():
    T = _coo()
    with pytest.raises(mx.MatrixExtraError, match="Can pass only one of 'binary' or 'logical'."):
        mx.as_coo_matrix(T, binary=True, logical=True)
    assert mx.as_coo_matrix(T) is T
    L = _coo(mx.lgTMatrix)
    assert mx.as_coo_matrix(L, logical=True) is L
    N = _coo(mx.ngTMatrix)
    assert mx.as_coo_matrix(N, binary=True) is N
    # a COO of another kind changes its value type entry by entry, without merging
    d = mx.as_coo_matrix(L)
    assert type(d) is mx.dgTMatrix and d.i is L.i
    assert d.x[:2].tolist() == [1.0, 0.0] and d.x.view(np.uint64)[2] == mx.NA_REAL.view(np.uint64)
    lo = mx.as_coo_matrix(T, logical=True)
    assert type(lo) is mx.lgTMatrix and lo.x.tolist() == [1, 1, 1, 1]
    assert mx.as_coo_matrix(N).x.tolist() == [1.0] * 4
    assert mx.as_coo_matrix(N, logical=True).x.tolist() == [1] * 4
    b = mx.as_coo_matrix(T, binary=True)
    assert type(b) is mx.ngTMatrix and b.x is None and b.j is T.j


def _csr():
    return mx.dgRMatrix(np.array([0, 1, 2, 3], np.int32), np.array([1, 0, 3], np.int32), np.array([1.0, 2.0, 3.0]),
                        (3, 4))


def _record(monkeypatch):
    calls = []

    def fake(name):
        def f(*a, **k):
            calls.append((name, a, k))
            return name
        return f
    for name in ["multiply_csr_by_coo", "add_csr_matrices", "logicalor_csr_matrices", "csr_op_vector",
                 "multiply_csr_by_csr"]:
        monkeypatch.setattr(operators, name, fake(name))
    return calls


def test_operator_dispatch_reaches_coo_paths(monkeypatch):
    calls = _record(monkeypatch)
    X, T = _csr(), _coo()
    assert X * T == "multiply_csr_by_coo" and calls[-1][1][:2] == (X, T) and calls[-1][2] == {"logical": False}
    assert T * X == "multiply_csr_by_coo" and calls[-1][1][:2] == (X, T)
    assert X & T == "multiply_csr_by_coo" and calls[-1][2] == {"logical": True}
    assert T & X == "multiply_csr_by_coo" and calls[-1][1][:2] == (X, T) and calls[-1][2] == {"logical": True}
    assert T + X == "add_csr_matrices" and calls[-1][1] == (X, T, False)          # add_csr_matrices(e2, e1)
    assert X + T == "add_csr_matrices" and calls[-1][1] == (X, T, False)
    assert T - X == "add_csr_matrices" and calls[-1][1] == (T, X, True)
    assert X - T == "add_csr_matrices" and calls[-1][1] == (X, T, True)
    assert T | X == "logicalor_csr_matrices" and calls[-1][1] == (T, X)
    assert X | T == "logicalor_csr_matrices" and calls[-1][1] == (X, T)
    v = np.array([1.0, 2.0, 3.0])
    for expr, op, lhs in [(lambda: T * v, "*", True), (lambda: v * T, "*", True), (lambda: T / v, "/", True),
                          (lambda: v / T, "/", False), (lambda: T ** v, "^", True), (lambda: T % v, "%%", True),
                          (lambda: T // v, "%/%", True), (lambda: T & v, "&", True)]:
        assert expr() == "csr_op_vector"
        assert calls[-1][1][0] is T and calls[-1][1][2] == op
        assert calls[-1][2].get("X_is_LHS", True) is lhs


def test_operator_dispatch_leaves_csr_paths_alone(monkeypatch):
    calls = _record(monkeypatch)
    X, Y = _csr(), _csr()
    v = np.array([1.0, 2.0, 3.0])
    assert X * Y == "multiply_csr_by_csr"
    assert X * v == "csr_op_vector" and calls[-1][1][0] is X
    assert X & v == "csr_op_vector"
    assert X + Y == "add_csr_matrices"
    assert not any(c[0] == "multiply_csr_by_coo" for c in calls)


def test_csc_or_coo_names_the_missing_class():
    C = mx.dgCMatrix(np.array([0, 1, 1, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.ones(3), (3, 4))
    with pytest.raises(mx.MatrixExtraError, match="lgCMatrix"):
        _coo() | C


@pytest.mark.skipif(_lib.load() is not None and __import__("conftest")._have_gpu(), reason="GPU present")
def test_coo_exports_fail_loudly_without_gpu():
    T = _coo()
    p = np.array([0, 1, 2, 3], np.int32)
    with pytest.raises(_lib.MxError):
        G.coo_to_csr(T.i, T.j, T.x, 3, 4)
    with pytest.raises(_lib.MxError):
        G.csr_to_coo(p)
    with pytest.raises(_lib.MxError):
        G.multiply_csr_by_coo_elemwise(p, np.array([1, 0, 3], np.int32), np.ones(3), T.i, T.j, T.x, 3, 4)
    with pytest.raises(_lib.MxError):
        G.logicaland_csr_by_coo_elemwise(p, np.array([1, 0, 3], np.int32), np.ones(3, np.int32), T.i, T.j,
                                         np.ones(4, np.int32), 3, 4)
    with pytest.raises(_lib.MxError):
        G.multiply_coo_by_dense_ignore_NAs_numeric(T.i, T.j, T.x, np.ones(3), 3, 4, 1, 0, 0, 0, 0, 1)
    with pytest.raises(_lib.MxError):
        G.multiply_coo_by_dense_ignore_NAs_logical(T.i, T.j, np.ones(4, np.int32), np.ones(3, np.int32), 3, 4)
    with pytest.raises(_lib.MxError):
        mx.as_csr_matrix(T)
    with pytest.raises(_lib.MxError):
        mx.as_coo_matrix(_csr())
