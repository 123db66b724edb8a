"""rbind / cbind mirror (matrixextra_amd/bind.py): everything that returns before a device call.  No GPU: a route
that would reach the device raises MxError here, which is how the routes are told apart."""
import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import bind, exports
from matrixextra_amd._lib import MxError
from matrixextra_amd.matrices import (MatrixExtraError, dgCMatrix, dgRMatrix, dgTMatrix, dsparseVector, lgRMatrix,
                                      lgTMatrix, lsparseVector, ngRMatrix, ngTMatrix, nsparseVector)


def csr(cls, nrow, ncol, Dimnames=None):
    """an nrow x ncol matrix with one entry in its first row (none without rows or columns)"""
    n = 1 if nrow and ncol else 0
    p = np.concatenate([[0], np.full(nrow, n)]).astype(np.int32)
    x = None if cls is ngRMatrix else np.ones(n, cls.value_dtype)
    return cls(p, np.zeros(n, np.int32), x, (nrow, ncol), Dimnames)


def coo(cls, nrow, ncol, Dimnames=None):
    n = 1 if nrow and ncol else 0
    x = None if cls is ngTMatrix else np.ones(n, cls.value_dtype)
    return cls(np.zeros(n, np.int32), np.zeros(n, np.int32), x, (nrow, ncol), Dimnames)


def test_the_new_names_are_exported():
    for name in ("rbind_csr", "rbind2", "cbind2", "rbind", "cbind"):
        assert getattr(mx, name) is getattr(bind, name)
    for name in ("rbind_coo", "cbind_csr_svec", "dense_to_svec", "concat_csr_batch"):
        assert callable(getattr(exports, name))


# ----------------------------------------------------------------------------------------------- rbind_csr shortcuts
def test_rbind_csr_of_nothing_and_of_rowless_matrices():
    out = mx.rbind_csr()                                                   # R/rbind.R:56-59
    assert type(out) is dgRMatrix and out.Dim == (0, 0) and out.p.tolist() == [0]
    out = mx.rbind_csr(csr(lgRMatrix, 0, 4), csr(ngRMatrix, 0, 7))         # ncols is the max over ALL operands (:43)
    assert type(out) is dgRMatrix and out.Dim == (0, 7) and out.j.size == 0


def test_rbind_csr_of_one_operand_returns_it_in_its_own_kind():
    for cls in (dgRMatrix, lgRMatrix, ngRMatrix):
        X = csr(cls, 3, 4)
        assert mx.rbind_csr(X) is X                                        # :60-61, cast_csr_same of a CSR
        assert mx.rbind_csr(csr(dgRMatrix, 0, 9), X, csr(ngRMatrix, 0, 2)) is X      # rowless operands are dropped first


def test_rbind_csr_of_two_operands_is_rbind2(monkeypatch):
    seen = []
    monkeypatch.setattr(bind, "rbind2", lambda x, y: seen.append((x, y)) or "two")
    X, Y = csr(dgRMatrix, 3, 4), csr(lgRMatrix, 2, 4)
    assert mx.rbind_csr(X, csr(dgRMatrix, 0, 4), Y) == "two" and seen == [(X, Y)]    # :62-63


def test_rbind_csr_early_return_without_columns():
    out = mx.rbind_csr(csr(lgRMatrix, 2, 0), csr(ngRMatrix, 3, 0), nsparseVector(np.zeros(0, np.int32), None, 0))
    assert type(out) is lgRMatrix and out.Dim == (6, 0)                    # :94-95, class by :66-75
    assert out.p.tolist() == [0] * 7 and out.j.size == 0 and out.x.size == 0 and out.Dimnames == [None, None]


@pytest.mark.parametrize("classes, want", [
    ((ngRMatrix, ngRMatrix, ngRMatrix), ngRMatrix), ((ngRMatrix, lgRMatrix, ngRMatrix), lgRMatrix),
    ((lgRMatrix, lgRMatrix, lgRMatrix), lgRMatrix), ((ngRMatrix, lgRMatrix, dgRMatrix), dgRMatrix)])
def test_rbind_csr_class_rule(classes, want):
    """:66-75, read off the early return: any numeric -> dgR, else any logical -> lgR, else ngR"""
    out = mx.rbind_csr(*[csr(c, 2, 0) for c in classes])
    assert type(out) is want and out.Dim == (6, 0)


def test_rbind_csr_int32_refusals(monkeypatch):
    monkeypatch.setattr(bind, "_INT_MAX", 7)
    three = [csr(dgRMatrix, 3, 2)] * 3
    with pytest.raises(MatrixExtraError, match="Result has too many rows for R to handle."):
        mx.rbind_csr(*three)                                               # 9 rows
    monkeypatch.setattr(bind, "_INT_MAX", 4)
    w = dsparseVector([1, 2], [1.0, 2.0], 2)
    with pytest.raises(MatrixExtraError, match="Result has too many non-zero entries for R to handle."):
        mx.rbind_csr(w, w.copy(), w.copy())                                # 3 rows pass, 6 entries do not


def test_rbind_csr_reaches_the_device_with_three_operands():
    with pytest.raises(MxError):
        mx.rbind_csr(csr(dgRMatrix, 2, 3), csr(dgRMatrix, 2, 3), csr(dgRMatrix, 2, 3))


# ----------------------------------------------------------------------------------------------- dimnames
def test_concat_dimname():
    f = bind.concat_dimname                                                # R/rbind.R:136-152
    assert f(None, None, 2, 3) is None
    assert f(["a", "b"], ["c"], 2, 1) == ["a", "b", "c"]
    assert f(None, ["c"], 2, 1) == ["", "", "c"]
    assert f(["a", "b"], None, 2, 3) == ["a", "b", "", "", ""]


def test_concat_dimnames():
    f = bind.concat_dimnames                                               # :154-186
    A = csr(dgRMatrix, 2, 2, [["r1", "r2"], ["a", "b"]])
    B = csr(dgRMatrix, 1, 3, [None, ["x", "y", "z"]])
    assert f(A, B) == [["r1", "r2", ""], ["a", "b", "z"]]                  # :159-161: the extra columns take y's names
    assert f(B, A) == [["", "r1", "r2"], ["x", "y", "z"]]
    assert f(csr(dgRMatrix, 2, 2), B) == [None, ["x", "y", "z"]]           # :166-167
    assert f(csr(dgRMatrix, 2, 2), csr(dgRMatrix, 1, 2)) == [None, None]
    assert f(A, csr(dgRMatrix, 1, 2)) == [["r1", "r2", ""], ["a", "b"]]
    with pytest.raises(MatrixExtraError, match="invalid 'times' argument"):           # :163 as written
        f(A, csr(dgRMatrix, 1, 3))


def test_cbind_dimnames_rule():
    f = bind._cbind_dimnames                                               # R/cbind.R:107-130
    A = csr(dgRMatrix, 2, 2, [["r1", "r2"], ["a", "b"]])
    B = csr(dgRMatrix, 3, 1, [["s1", "s2", "s3"], ["c"]])
    assert f(A, B) == [["r1", "r2", "s1"], ["a", "b", "c"]]                # :114 as written: y's FIRST names fill up
    assert f(B, A) == [["s1", "s2", "s3"], ["c", "a", "b"]]
    assert f(A, csr(dgRMatrix, 3, 1)) == [["r1", "r2", ""], ["a", "b"]]    # :123 as written: no "" for y's column
    assert f(csr(dgRMatrix, 3, 1), A) == [["r1", "r2", ""], ["", "a", "b"]]          # :117-121, :127-128
    assert f(csr(dgRMatrix, 2, 2), csr(dgRMatrix, 3, 1)) == [None, None]


# ----------------------------------------------------------------------------------------------- shortcuts of the pairs
def test_rbind2_zero_row_shortcuts():
    X, E = csr(lgRMatrix, 3, 2, [["a", "b", "c"], None]), csr(dgRMatrix, 0, 5)
    for out in (mx.rbind2(E, X), mx.rbind2(X, E)):                         # R/rbind.R:254-265
        assert type(out) is lgRMatrix and out.Dim == (3, 5) and out.p is X.p and out.Dimnames[0] == ["a", "b", "c"]
    assert X.Dim == (3, 2)
    T, ET = coo(ngTMatrix, 2, 3), coo(dgTMatrix, 0, 6)
    for out in (mx.rbind2(ET, T), mx.rbind2(T, ET)):                       # :407-418
        assert type(out) is ngTMatrix and out.Dim == (2, 6) and out.i is T.i
    C = dgCMatrix(np.zeros(3, np.int32), np.zeros(0, np.int32), np.zeros(0), (4, 2))
    out = mx.rbind2(E, C)                                                  # y is returned in its own class
    assert type(out) is dgCMatrix and out.Dim == (4, 5) and out.p.size == 6


def test_cbind_csr_zero_column_shortcuts():
    X, E = csr(ngRMatrix, 2, 3), csr(dgRMatrix, 5, 0)
    for out in (mx.cbind2(E, X), mx.cbind2(X, E)):                         # R/cbind.R:59-70
        assert type(out) is ngRMatrix and out.Dim == (5, 3) and out.p.tolist() == [0, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("x, y, want", [
    (ngRMatrix, ngRMatrix, "n"), (ngRMatrix, lgRMatrix, "l"), (lgRMatrix, ngRMatrix, "l"), (lgRMatrix, lgRMatrix, "l"),
    (dgRMatrix, ngRMatrix, "d"), (lgRMatrix, dgRMatrix, "d"), (dgRMatrix, dgRMatrix, "d"),
    (ngTMatrix, ngTMatrix, "n"), (lgTMatrix, ngTMatrix, "l"), (dgTMatrix, lgTMatrix, "d")])
def test_kind_rule_of_the_pairs(x, y, want):
    """R/rbind.R:311-317, :430-436, R/cbind.R:82-99"""
    make = csr if issubclass(x, mx.RsparseMatrix) else coo
    assert bind._kind2(make(x, 2, 2), make(y, 2, 2)) == want


def test_kind_rule_with_sparse_vectors():
    n, l, d = nsparseVector([1], None, 2), lsparseVector([1], [1], 2), dsparseVector([1], [1.0], 2)
    assert bind._kind2(n, csr(ngRMatrix, 2, 2)) == "n" and bind._kind2(csr(ngRMatrix, 2, 2), l) == "l"
    assert bind._kind2(l, n) == "l" and bind._kind2(d, n) == "d"
    assert bind._kind2(mx.isparseVector([1], [1], 2), n) == "d"            # an isparseVector is numeric


# ----------------------------------------------------------------------------------------------- refusals
def test_dense_vector_refusals():
    X = csr(dgRMatrix, 3, 4)
    with pytest.raises(MatrixExtraError, match=r"rbind2: the vector has length 3, which is neither 1 nor .*\(4\)"):
        mx.rbind2(X, np.ones(3))
    with pytest.raises(MatrixExtraError, match=r"cbind2: the vector has length 4, which is neither 1 nor .*\(3\)"):
        mx.cbind2(np.ones(4), X)
    with pytest.raises(MatrixExtraError, match=r"rbind2: no method for \(dgTMatrix, ndarray\)"):
        mx.rbind2(coo(dgTMatrix, 3, 4), np.ones(4))                        # the reference has no T / dense method
    with pytest.raises(MatrixExtraError, match="cbind2: no method"):
        mx.cbind2(np.ones(3), coo(dgTMatrix, 3, 4))
    with pytest.raises(MatrixExtraError, match="no method"):
        mx.rbind2(np.ones(3), np.ones(3))
    with pytest.raises(MatrixExtraError, match="no method"):
        mx.cbind2(X, "a")


def test_invalid_operands_are_refused_before_the_device():
    bad = dgRMatrix(np.array([0, 1], np.int32), np.zeros(1, np.int32), np.ones(1), (3, 2))
    with pytest.raises(MatrixExtraError, match="'p' doesn't match with dimension"):
        mx.rbind_csr(bad, csr(dgRMatrix, 1, 2), csr(dgRMatrix, 1, 2))
    with pytest.raises(MatrixExtraError, match="'p' doesn't match with dimension"):
        mx.cbind2(bad, csr(dgRMatrix, 3, 2))
    with pytest.raises(MatrixExtraError, match="'p' doesn't match with dimension"):
        mx.rbind2(csr(dgRMatrix, 3, 2), bad)


def test_the_vector_column_export_checks_the_vector_before_the_device():
    p, j = np.array([0, 1, 1], np.int32), np.zeros(1, np.int32)
    for vi, message in (([1, 3], "outside 1..length"), ([0, 1], "outside 1..length"), ([2, 1, 2], "stores a position twice")):
        with pytest.raises(MxError, match=message):
            exports.cbind_csr_svec(p, j, np.ones(1), 4, 0, np.array(vi, np.int32), np.ones(len(vi)), 3, 2, False, 0)
    with pytest.raises(MxError, match="bad kind"):
        exports.cbind_csr_svec(p, j, np.ones(1), 4, 0, np.array([1], np.int32), np.ones(1), 2, 2, False, 0)


def test_too_many_columns_is_refused(monkeypatch):
    monkeypatch.setattr(bind, "_INT_MAX", 5)
    with pytest.raises(MatrixExtraError, match="too many columns"):
        mx.cbind2(csr(dgRMatrix, 2, 3), csr(dgRMatrix, 2, 3))


# ----------------------------------------------------------------------------------------------- the folds
def test_rbind_and_cbind_are_left_folds(monkeypatch):
    calls = []
    monkeypatch.setattr(bind, "rbind2", lambda x, y: calls.append(("r", x, y)) or f"({x}{y})")
    monkeypatch.setattr(bind, "cbind2", lambda x, y: calls.append(("c", x, y)) or f"[{x}{y}]")
    assert mx.rbind("a", "b", "c", "d") == "(((ab)c)d)"
    assert mx.cbind("a", "b", "c") == "[[ab]c]"
    assert calls == [("r", "a", "b"), ("r", "(ab)", "c"), ("r", "((ab)c)", "d"), ("c", "a", "b"), ("c", "[ab]", "c")]
    assert mx.rbind("a") == "a" and mx.cbind() is None and len(calls) == 5
