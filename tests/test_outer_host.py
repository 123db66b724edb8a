"""What the `%*%` / tcrossprod / crossprod dispatch decides for the outer products and the float32 vector forms before a
device call (R/matmul.R:220-262, 327-367, 405-427, 480-500, 659-751): taken only under options["mxgpu.outer_route"];
which export each operand class reaches and with which arguments, and the class, Dim and Dimnames of the result.  The
exports are replaced, so no GPU is needed."""
import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G, matmul, matrices

OPTION = "mxgpu.outer_route"
NA = mx.NA_INTEGER
OUTER_EXPORTS = ["matmul_colvec_by_scolvecascsr", "matmul_colvec_by_scolvecascsr_f32", "matmul_rowvec_by_csc",
                 "matmul_rowvec_by_cscbin"] + ["matmul_spcolvec_by_scolvecascsr_" + k
                                               for k in ("numeric", "integer", "logical", "binary")]


class Names(np.ndarray):
    """a numeric vector with names(y)"""
    names = None


def named(values, names):
    v = np.asarray(values, dtype=np.float64).view(Names)
    v.names = list(names)
    return v


@pytest.fixture
def calls(monkeypatch):
    """every outer export records its arguments and returns a recognisable triple / row; everything else that would
    reach the device fails the test, except the sort of a sparse vector, which is recorded and done in numpy"""
    seen = []

    def triple(name):
        def f(*args):
            seen.append((name, args))
            return dict(indptr=np.array([0, 2, 2], np.int32), indices=np.array([0, 1], np.int32), values=np.array([7.0, 8.0]))
        return f

    def row(name):
        def f(*args):
            seen.append((name, args))
            return np.array([[1.5, 2.5]], dtype=np.float32)
        return f

    for name in OUTER_EXPORTS:
        monkeypatch.setattr(G, name, row(name) if "rowvec" in name else triple(name))

    def sort_vec(i, x=None):
        seen.append(("sort", (i,)))
        o = np.argsort(i, kind="stable")
        i[:] = i[o]
        if x is not None:
            x[:] = x[o]

    for k in ("numeric", "integer", "logical"):
        monkeypatch.setattr(G, "sort_vector_indices_" + k, sort_vec)
    monkeypatch.setattr(G, "sort_vector_indices_binary", sort_vec)
    monkeypatch.setattr(G, "check_valid_svec", lambda ii, n: {})

    def reached(*a, **k):
        raise AssertionError("another device route was reached")
    for name in ("matmul_csr_dvec_numeric", "matmul_csr_dvec_float32", "matmul_csr_svec_numeric",
                 "matmul_dense_csc_float32", "tcrossprod_dense_csr_float32"):
        monkeypatch.setattr(G, name, reached)
    monkeypatch.setitem(matrices.options, OPTION, True)
    return seen


def one_col():
    return mx.dgRMatrix([0, 1, 1], [0], [2.0], (2, 1), [["a", "b"], None])


def test_option_is_off_by_default_and_the_refusals_hold(monkeypatch):
    assert not matrices.options.get(OPTION, False)
    for name in OUTER_EXPORTS:
        monkeypatch.setattr(G, name, lambda *a: pytest.fail("an outer export was reached without the option"))
    monkeypatch.setattr(G, "matmul_csr_dvec_numeric", lambda *a: pytest.fail("a device route was reached"))
    monkeypatch.setattr(G, "check_valid_svec", lambda ii, n: {})
    X = one_col()
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        X @ mx.dsparseVector([1], [1.0], 1)
    with pytest.raises(mx.MatrixExtraError, match="outer product"):
        matmul.matmul(X, mx.nsparseVector([1], None, 3))
    with pytest.raises(mx.MatrixExtraError, match="Matrix-vector dimensions do not match."):
        X @ np.array([1.0, 2.0, 3.0])
    with pytest.raises(mx.MatrixExtraError, match="Matrix-vector dimensions do not match."):
        X @ mx.float32(np.ones(3, np.float32))
    with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for crossprod"):
        mx.crossprod(mx.float32(np.ones(2, np.float32)), mx.dgCMatrix([0, 1], [0], [1.0], (2, 1)))


def test_entry_points_declared():
    wanted = {"mxd_csr_outer_dense_workspace_bytes", "mxd_csr_outer_dense_count", "mxd_csr_outer_dense_fill",
              "mxd_csr_outer_svec_workspace_bytes", "mxd_csr_outer_svec_count", "mxd_csr_outer_svec_fill",
              "mxd_rowvec_by_csc", "mx_matmul_colvec_by_scolvecascsr_begin",
              "mx_matmul_spcolvec_by_scolvecascsr_begin", "mx_matmul_rowvec_by_csc"}
    assert wanted <= set(_lib.declared_symbols())
    for name in OUTER_EXPORTS:
        assert callable(getattr(G, name))
    assert callable(matmul.outerprod_csrsinglecol_by_dvec)


def test_dense_vector_reaches_the_f64_outer_product(calls):
    X = one_col()
    out = X @ named([1.0, 2.0, 3.0], "xyz")
    (name, args), = calls
    assert name == "matmul_colvec_by_scolvecascsr"
    assert args[0].dtype == np.float64 and list(args[0]) == [1.0, 2.0, 3.0]
    assert args[1] is X.p and args[2] is X.j and args[3] is X.x
    assert type(out) is mx.dgRMatrix and out.Dim == (2, 3) and out.Dimnames == [["a", "b"], list("xyz")]
    assert list(out.p) == [0, 2, 2] and list(out.j) == [0, 1] and list(out.x) == [7.0, 8.0]
    del calls[:]
    out = X @ np.array([1, NA], dtype=np.int32)                     # mode(y) <- "double": NA_integer_ -> NA_real_
    assert calls[0][1][0][0] == 1.0 and calls[0][1][0][1:].view(np.uint64)[0] == 0x7FF00000000007A2
    assert out.Dim == (2, 2) and out.Dimnames == [["a", "b"], None]
    del calls[:]
    X @ np.array([True, False])
    assert calls[0][0] == "matmul_colvec_by_scolvecascsr" and list(calls[0][1][0]) == [1.0, 0.0]


def test_other_matrix_classes_are_normalised(calls):
    L = mx.lgRMatrix([0, 1, 2], [0, 0], [1, NA], (2, 1))
    L @ np.array([2.0])
    x = calls[0][1][3]
    assert x.dtype == np.float64 and x[0] == 1.0 and np.isnan(x[1])
    del calls[:]
    mx.ngRMatrix([0, 1, 1], [0], None, (2, 1)) @ np.array([2.0])
    assert list(calls[0][1][3]) == [1.0]
    with pytest.raises(mx.MatrixExtraError, match="Internal error"):
        matmul.outerprod_csrsinglecol_by_dvec(mx.dgRMatrix([0, 1], [1], [1.0], (1, 2)), np.ones(2))


@pytest.mark.parametrize("cls, kind, x", [(mx.dsparseVector, "numeric", [2.5, -1.0]), (mx.isparseVector, "integer", [4, NA]),
                                           (mx.lsparseVector, "logical", [1, NA]), (mx.nsparseVector, "binary", None)])
def test_sparse_vector_classes(calls, cls, kind, x):
    X = one_col()
    y = cls([3, 1], x, 5)                                           # unsorted
    out = X @ y
    assert calls[0][0] == "sort"
    name, args = calls[1]
    assert name == "matmul_spcolvec_by_scolvecascsr_" + kind
    assert args[0] is X.p and args[1] is X.j and args[2] is X.x
    assert list(args[3]) == [1, 3] and args[3].dtype == np.int32    # 1-based y@i, sorted
    assert args[-1] == 5                                            # y@length
    if x is not None:
        assert list(args[4]) == list(reversed(x))                   # the values follow the sort
    assert list(y.i) == [3, 1]                                      # a copy was sorted
    assert type(out) is mx.dgCMatrix and out.Dim == (2, 5) and out.Dimnames == [["a", "b"], None]
    assert list(out.p) == [0, 2, 2] and list(out.i) == [0, 1] and list(out.x) == [7.0, 8.0]


def test_inplace_sort_sorts_the_vector_itself(calls, monkeypatch):
    monkeypatch.setitem(matrices.options, "MatrixExtra.inplace_sort", True)
    y = mx.dsparseVector([3, 1], [2.5, -1.0], 3)
    one_col() @ y
    assert list(y.i) == [1, 3] and list(y.x) == [-1.0, 2.5]


def test_other_sparse_vector_classes_fall_back_to_dsparseVector(calls):
    class zsparseVector(mx.sparseVector):
        value_dtype = np.float64
        r_class = "zsparseVector"
    out = matmul.matmul(one_col(), zsparseVector([2], [3.0], 2))
    name, args = calls[-1]
    assert name == "matmul_spcolvec_by_scolvecascsr_numeric" and list(args[3]) == [2] and list(args[4]) == [3.0]
    assert type(out) is mx.dgCMatrix and out.Dim == (2, 2)


def test_float32_vector_on_the_right(calls):
    X = one_col()
    y = mx.float32(np.array([1.5, 2.0, -3.0], np.float32))
    out = X @ y
    (name, args), = calls
    assert name == "matmul_colvec_by_scolvecascsr_f32"
    assert args[0].dtype == np.float32 and args[0].tobytes() == np.array([1.5, 2.0, -3.0], np.float32).tobytes()
    assert args[1] is X.p and args[2] is X.j and args[3] is X.x
    assert type(out) is mx.dgRMatrix and out.Dim == (2, 3) and out.Dimnames == [["a", "b"], None]


def test_float32_vector_times_one_row_csc(calls):
    Y = mx.dgCMatrix([0, 1, 1, 2], [0, 0], [2.0, 3.0], (1, 3), [None, list("pqr")])
    x = mx.float32(np.array([1.0, 2.0], np.float32))
    out = x @ Y
    (name, args), = calls
    assert name == "matmul_colvec_by_scolvecascsr_f32" and args[0].dtype == np.float32
    assert args[1] is Y.p and args[2] is Y.i and args[3] is Y.x
    assert type(out) is mx.dgCMatrix and out.Dim == (2, 3) and out.Dimnames == [None, list("pqr")]


def test_float32_row_vector_times_csc(calls):
    Y = mx.dgCMatrix([0, 1, 3], [0, 0, 1], [2.0, 3.0, 4.0], (2, 2))
    x = mx.float32(np.array([1.0, 2.0], np.float32))
    out = x @ Y
    (name, args), = calls
    assert name == "matmul_rowvec_by_csc" and args[0].dtype == np.float32 and list(args[0]) == [1.0, 2.0]
    assert args[1] is Y.p and args[2] is Y.i and args[3] is Y.x
    assert type(out) is mx.float32 and out.Data.shape == (1, 2) and list(out.Data[0]) == [1.5, 2.5]
    with pytest.raises(mx.MatrixExtraError, match=r"\(row\) vector-Matrix multiplication dimensions do not match."):
        mx.float32(np.ones(3, np.float32)) @ Y
    del calls[:]
    out = mx.crossprod(x, Y)
    assert calls[0][0] == "matmul_rowvec_by_csc" and type(out) is mx.float32
    with pytest.raises(mx.MatrixExtraError, match=r"\(column\) vector-Matrix crossprod dimensions do not match."):
        mx.crossprod(mx.float32(np.ones(3, np.float32)), Y)


def test_float32_vector_tcrossprod_csr(calls):
    x = mx.float32(np.array([1.0, 2.0], np.float32))
    col = mx.dgRMatrix([0, 1, 1, 2], [0, 0], [2.0, 3.0], (3, 1))
    out = mx.tcrossprod(x, col)                                       # one column: the outer product
    (name, args), = calls
    assert name == "matmul_colvec_by_scolvecascsr_f32" and args[1] is col.p and args[2] is col.j
    assert type(out) is mx.dgCMatrix and out.Dim == (2, 3)
    del calls[:]
    Y = mx.dgRMatrix([0, 1, 3], [0, 0, 1], [2.0, 3.0, 4.0], (2, 2))
    out = mx.tcrossprod(x, Y)
    assert calls[0][0] == "matmul_rowvec_by_csc" and calls[0][1][1] is Y.p and calls[0][1][2] is Y.j
    assert type(out) is mx.float32 and out.Data.shape == (1, 2)
    del calls[:]
    N = mx.ngRMatrix([0, 1, 3], [0, 0, 1], None, (2, 2))
    mx.tcrossprod(x, N)
    assert calls[0][0] == "matmul_rowvec_by_cscbin" and len(calls[0][1]) == 3


def test_wider_matrices_keep_their_routes(calls, monkeypatch):
    X = mx.dgRMatrix([0, 1, 2], [0, 1], [1.0, 2.0], (2, 2))
    monkeypatch.setattr(G, "matmul_csr_dvec_numeric", lambda p, j, x, y, n: np.array([5.0, 6.0]))
    monkeypatch.setattr(G, "matmul_csr_dvec_float32", lambda p, j, x, y, n: np.array([5.0, 6.0], np.float32))
    assert np.asarray(X @ np.ones(2)).shape == (2, 1)
    assert (X @ mx.float32(np.ones(2, np.float32))).Data.shape == (2, 1)
    assert calls == []
