"""CSC * dense checks that need no GPU: what multiply_csc_by_dense_internal (R/operators.R:568-661) decides before a
device call (the dimension message, the float32-vector branches and the routes that go to Matrix's own methods),
`&` and vectors on a dgCMatrix, the operator dispatch of `C * M`, `M * C`, `float32 * C`, and the new C-ABI entries
(declared and exported)."""
import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G, operators

DIM = "Matrices must have the same dimensions in order to multiply them."
ROUTES = ["multiply_csc_by_dense_ignore_NAs_numeric", "multiply_csc_by_dense_ignore_NAs_float32",
          "multiply_csc_by_dense_ignore_NAs_integer", "multiply_csc_by_dense_ignore_NAs_logical",
          "logicaland_csc_by_dense_ignore_NAs", "multiply_csc_by_dense_keep_NAs_numeric",
          "multiply_csc_by_dense_keep_NAs_integer", "multiply_csc_by_dense_keep_NAs_logical",
          "multiply_csc_by_dense_keep_NAs_float32"]


def _csc(ncol=2):
    """3 x ncol: column 0 holds rows 0 and 2, column 1 row 1, later columns nothing."""
    p = np.array([0, 2, 3] + [3] * (ncol - 2), np.int32)[:ncol + 1]
    nnz = int(p[-1])
    return mx.dgCMatrix(p, np.array([0, 2, 1], np.int32)[:nnz], np.array([1.0, 2.0, 3.0])[:nnz], (3, ncol))


@pytest.fixture
def no_device(monkeypatch):
    """every route that would reach the device fails the test"""
    def reached(*a, **k):
        raise AssertionError("a device route was reached")
    for name in ROUTES + ["sort_sparse_indices_inplace"]:
        monkeypatch.setattr(G, name, reached)


@pytest.fixture(params=[False, True], ids=["keep_na", "ignore_na"])
def ignore_na(request):
    old = mx.options.get("MatrixExtra.ignore_na")
    mx.options["MatrixExtra.ignore_na"] = request.param
    yield request.param
    if old is None:
        del mx.options["MatrixExtra.ignore_na"]
    else:
        mx.options["MatrixExtra.ignore_na"] = old


def test_entry_points_declared_and_exported():
    wanted = {"mx_" + r for r in ROUTES} | {"mxd_csc_by_dense_elemwise", "mxd_csc_dense_na_workspace_bytes",
                                             "mxd_csc_dense_na_count", "mxd_csc_dense_na_fill"}
    header = open(_lib.HEADER_PATH).read()
    assert all(s + "(" in header for s in wanted)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in wanted)
    assert not hasattr(lib, "mx_logicaland_csc_by_dense_keep_NAs")                    # not ported


def test_dimension_message(no_device, ignore_na):
    C = _csc()
    for other in (np.ones((2, 2)), np.ones((3, 3), np.int32), np.ones((3, 1), bool), mx.DenseMatrix(np.ones((4, 2))),
                  mx.float32(np.ones((2, 2), np.float32))):
        with pytest.raises(mx.MatrixExtraError, match=DIM):
            C * other
        with pytest.raises(mx.MatrixExtraError, match=DIM):
            other * C


def test_float32_vector_branches(no_device, ignore_na):
    C = _csc()                                                       # 3 x 2
    empty = C * mx.float32(np.zeros(0, np.float32))                  # :573-578: numeric()
    assert isinstance(empty, np.ndarray) and empty.dtype == np.float64 and empty.size == 0
    with pytest.raises(mx.MatrixExtraError, match="Vector to multiply with has more entries than matrix dimensions."):
        C * mx.float32(np.ones(7, np.float32))
    for n2 in (4, 5, 6, 2, 1):                                       # longer or shorter than nrow: e1 * float::dbl(e2)
        with pytest.raises(mx.MatrixExtraError, match=r"R/operators.R:585"):
            C * mx.float32(np.ones(n2, np.float32))
        with pytest.raises(mx.MatrixExtraError, match=r"R/operators.R:585"):
            mx.float32(np.ones(n2, np.float32)) * C
    # nrow entries: recycled down one column (nrow * ncol rows), so a two-column e1 fails the dimension check (sic)
    with pytest.raises(mx.MatrixExtraError, match=DIM):
        C * mx.float32(np.array([1.0, np.nan, 3.0], np.float32))


def test_recycle_float32_vector():
    v = mx.float32(np.array([1.0, 2.0, 3.0], np.float32))
    r = operators._recycle_float32_vector(_csc(2), v)
    assert r.Data.shape == (6, 1)
    np.testing.assert_array_equal(r.Data.reshape(-1), [1, 2, 3, 1, 2, 3])
    r1 = operators._recycle_float32_vector(_csc(1), v)
    assert r1.Data.shape == (3, 1) and not r1.is_vector


def test_ampersand_raises_lgCMatrix(no_device):
    C = _csc()
    M = np.ones((3, 2), bool)
    for f in (lambda: C & M, lambda: M & C, lambda: C & mx.float32(np.ones((3, 2), np.float32)),
              lambda: mx.float32(np.ones((3, 2), np.float32)) & C):
        with pytest.raises(mx.MatrixExtraError, match="would give an lgCMatrix, which this package does not provide"):
            f()


def test_vectors_and_scalars_raise(no_device):
    C = _csc()
    for f in (lambda: C * np.ones(3), lambda: np.ones(3) * C, lambda: C * 2.0, lambda: 2.0 * C,
              lambda: C * np.ones((3, 2, 1))):
        with pytest.raises(mx.MatrixExtraError, match="Matrix's own method"):
            f()


def test_operand_orders_dispatch_to_the_same_function(monkeypatch):
    seen = []
    monkeypatch.setattr(operators, "multiply_csc_by_dense", lambda e1, e2: seen.append((e1, e2)) or "done")
    C = _csc()
    M = np.ones((3, 2))
    Dm = mx.DenseMatrix(np.ones((3, 2)))
    F = mx.float32(np.ones((3, 2), np.float32))
    assert C * M == "done" and M * C == "done" and Dm * C == "done" and C * F == "done" and F * C == "done"
    assert [(a is C, b is o) for (a, b), o in zip(seen, (M, M, Dm, F, F))] == [(True, True)] * 5


def test_dense_operand_kinds():
    k = lambda a: operators._csc_dense_operand(a)[1]                 # noqa: E731
    assert k(np.ones((2, 2))) == "numeric"
    assert k(np.ones((2, 2), np.int32)) == "integer"
    assert k(np.ones((2, 2), bool)) == "logical"
    assert k(mx.RLogical(np.ones((2, 2), np.int32))) == "logical"
    assert k(mx.float32(np.ones((2, 2), np.float32))) == "float32"
    for other in (np.ones((2, 2), np.int64), np.ones((2, 2), np.float32), np.ones((2, 2), np.int16)):
        a, kind = operators._csc_dense_operand(other)               # mode(e2) <- "double"
        assert kind == "numeric" and a.dtype == np.float64
