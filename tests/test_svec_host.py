"""sparseVector checks that need no GPU: the objects and as_sparse_vector (R/conversions.R:593-619), the validation
messages of R/utils.R:456-466, what multiply_csr_by_svec_elemwise_internal (R/operators.R:1564-1589) and the `%*%`
dispatch decide before a device call, and the new C-ABI entries (declared and, when the library is built, exported)."""
import os

import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G, matmul, operators

NA = mx.NA_INTEGER
DEVICE_ROUTES = ["multiply_csr_by_svec_no_NAs", "multiply_csr_by_svec_keep_NAs", "sort_vector_indices_numeric",
                 "sort_vector_indices_integer", "sort_vector_indices_logical", "sort_vector_indices_binary",
                 "sort_sparse_indices_inplace", "check_valid_svec", "matmul_csr_svec_numeric"]


@pytest.fixture
def no_device(monkeypatch):
    """every route that would reach the device fails the test"""
    def reached(*a, **k):
        raise AssertionError("a device route was reached")
    for name in DEVICE_ROUTES:
        monkeypatch.setattr(G, name, reached)


def _X():
    return mx.dgRMatrix([0, 2, 3, 3, 4], [0, 2, 1, 0], [1.0, 2.0, 3.0, 4.0], (4, 3), [list("abcd"), None])


def test_entry_points_declared_and_exported():
    wanted = {"mx_multiply_csr_by_svec_begin", "mx_sort_vector_indices", "mxd_csr_by_svec_workspace_bytes",
              "mxd_csr_by_svec_count", "mxd_csr_by_svec_fill", "mxd_sort_vector_indices",
              "mxd_sort_vector_indices_workspace_bytes"}
    header = open(_lib.HEADER_PATH).read()
    assert all(s + "(" in header for s in wanted)
    assert wanted <= set(_lib.declared_symbols())
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, s) for s in wanted)
        assert lib.mxd_csr_by_svec_workspace_bytes(1000) >= 4 * 1000 + 16
    for name in DEVICE_ROUTES[:6]:
        assert callable(getattr(G, name))


def test_objects():
    v = mx.dsparseVector([3, 1], [2.5, -1.0], 5)
    assert isinstance(v, mx.sparseVector) and len(v) == 5 and v.length == 5
    assert v.i.dtype == np.int32 and v.x.dtype == np.float64 and v.has_x()
    np.testing.assert_array_equal(v.toarray(), [-1.0, 0, 2.5, 0, 0])
    c = v.copy()
    assert c.i is not v.i and c.x is not v.x and list(c.i) == [3, 1] and len(c) == 5
    i = mx.isparseVector([2], [NA], 2)
    assert i.x.dtype == np.int32 and np.isnan(i.toarray()[1])
    assert mx.lsparseVector([1], [1], 3).x.dtype == np.int32
    n = mx.nsparseVector([2, 4], None, 4)
    assert n.x is None and not n.has_x() and list(n.toarray()) == [0, 1, 0, 1]
    assert len(mx.dsparseVector([], [], 0)) == 0
    assert "dsparseVector of length 5" in repr(v)


def test_as_sparse_vector_from_dense():
    v = mx.as_sparse_vector(np.array([0.0, 1.5, 0.0, np.nan, -2.0]))
    assert type(v) is mx.dsparseVector and list(v.i) == [2, 4, 5] and len(v) == 5
    assert v.x[0] == 1.5 and np.isnan(v.x[1]) and v.x[2] == -2.0
    M = np.array([[1.0, 0.0, 3.0], [0.0, 2.0, 0.0]])                # column-major cells 1, 4, 5
    assert list(mx.as_sparse_vector(M).i) == [1, 4, 5] and list(mx.as_sparse_vector(M).x) == [1.0, 2.0, 3.0]
    f = mx.as_sparse_vector(mx.float32(M.astype(np.float32)))
    assert type(f) is mx.dsparseVector and list(f.i) == [1, 4, 5] and len(f) == 6
    i = mx.as_sparse_vector(np.array([0, 7, NA], np.int32), integer=True)
    assert type(i) is mx.isparseVector and list(i.i) == [2, 3] and list(i.x) == [7, NA]
    b = mx.as_sparse_vector(np.array([True, False, True]), logical=True)
    assert type(b) is mx.lsparseVector and list(b.i) == [1, 3] and list(b.x) == [1, 1]
    assert type(mx.as_sparse_vector(np.array([True, False]))) is mx.dsparseVector
    n = mx.as_sparse_vector(np.array([0.0, 2.0]), binary=True)
    assert type(n) is mx.nsparseVector and list(n.i) == [2] and n.x is None


def test_as_sparse_vector_from_sparse_matrices():
    X = _X()
    v = mx.as_sparse_vector(X)                                      # cells (0,0) (3,0) (1,1) (0,2) column-major
    assert type(v) is mx.dsparseVector and len(v) == 12
    assert list(v.i) == [1, 4, 6, 9] and list(v.x) == [1.0, 4.0, 3.0, 2.0]
    row = mx.dgRMatrix([0, 2], [0, 2], [5.0, 6.0], (1, 4))          # a CSR row
    assert list(mx.as_sparse_vector(row).i) == [1, 3] and len(mx.as_sparse_vector(row)) == 4
    col = mx.dgRMatrix([0, 0, 1, 2], [0, 0], [5.0, 6.0], (3, 1))    # a CSR column
    assert list(mx.as_sparse_vector(col).i) == [2, 3] and list(mx.as_sparse_vector(col).x) == [5.0, 6.0]
    assert type(mx.as_sparse_vector(mx.ngRMatrix([0, 1], [1], None, (1, 2)))) is mx.dsparseVector
    assert type(mx.as_sparse_vector(mx.ngRMatrix([0, 1], [1], None, (1, 2)), binary=True)) is mx.nsparseVector
    lg = mx.as_sparse_vector(mx.lgRMatrix([0, 2], [0, 1], [1, NA], (1, 2)), logical=True)
    assert type(lg) is mx.lsparseVector and list(lg.x) == [1, NA]
    C = mx.dgCMatrix([0, 1, 3], [1, 0, 1], [7.0, 8.0, 9.0], (2, 2))
    assert list(mx.as_sparse_vector(C).i) == [2, 3, 4] and list(mx.as_sparse_vector(C).x) == [7.0, 8.0, 9.0]


def test_as_sparse_vector_kind_changes():
    i = mx.isparseVector([1, 3], [NA, 4], 3)
    d = mx.as_sparse_vector(i)
    assert type(d) is mx.dsparseVector and d.x[1] == 4.0
    assert d.x[:1].view(np.uint64)[0] == 0x7FF00000000007A2         # NA_integer_ -> NA_real_
    lg = mx.lsparseVector([2], [NA], 2)
    assert mx.as_sparse_vector(lg).x.view(np.uint64)[0] == 0x7FF00000000007A2
    assert mx.as_sparse_vector(d) is d
    back = mx.as_sparse_vector(d, integer=True)
    assert type(back) is mx.isparseVector and list(back.x) == [NA, 4]
    assert list(mx.as_sparse_vector(mx.dsparseVector([1, 2], [0.0, np.nan], 2), logical=True).x) == [0, NA]
    n = mx.nsparseVector([2, 3], None, 3)
    assert list(mx.as_sparse_vector(n).x) == [1.0, 1.0] and mx.as_sparse_vector(n, binary=True) is n
    for kw in (dict(binary=True, logical=True), dict(logical=True, integer=True), dict(binary=True, integer=True)):
        with pytest.raises(mx.MatrixExtraError, match="Can pass at most one of 'binary', 'logical', 'integer'."):
            mx.as_sparse_vector(d, **kw)


def test_validation_messages(no_device):
    v = mx.dsparseVector([1], [1.0], 3)
    v.length = -1
    with pytest.raises(mx.MatrixExtraError, match="Vector has negative length."):
        mx.check_valid_matrix(v)
    v.length = None
    with pytest.raises(mx.MatrixExtraError, match="Vector has invalid length."):
        mx.check_valid_matrix(v)
    w = mx.dsparseVector([1, 2], [1.0], 3)
    with pytest.raises(mx.MatrixExtraError, match="Vector indices and values have different length."):
        mx.check_valid_matrix(w)


def test_branches_before_the_device(no_device):
    X = _X()
    empty = X * mx.dsparseVector([], [], 0)                          # R/operators.R:1565-1566: numeric()
    assert isinstance(empty, np.ndarray) and empty.dtype == np.float64 and empty.size == 0
    assert mx.dsparseVector([], [], 0) * X is not None
    assert X * mx.nsparseVector([1, 2, 3, 4], None, 4) is X         # :1579: every position stored, no values
    assert mx.nsparseVector([2, 1], None, 2) * X is X
    for v in (mx.dsparseVector([1], [2.0], 3), mx.dsparseVector([1], [2.0], 8), mx.nsparseVector([5], None, 5)):
        with pytest.raises(mx.MatrixExtraError, match="R/operators.R:1587-1588"):
            X * v
        with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
            v * X


def test_dense_vector_routes_keep_their_refusals(monkeypatch):
    """length 1 and every-position-stored vectors go to csr_op_vector unchanged, with its own NA refusal"""
    X = _X()
    seen = []
    monkeypatch.setattr(operators, "csr_op_vector", lambda e1, e2, op: seen.append((e1, np.asarray(e2), op)) or "done")
    assert X * mx.dsparseVector([1], [2.5], 1) == "done"
    assert seen[-1][0] is X and list(seen[-1][1]) == [2.5] and seen[-1][2] == "*"
    assert X * mx.isparseVector([], [], 1) == "done" and list(seen[-1][1]) == [0.0]
    monkeypatch.undo()
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        X * mx.dsparseVector([1], [np.nan], 1)                      # multiply_csr_by_dvec_with_NAs stays out


def test_matmul_dispatch(no_device):
    X = _X()
    with pytest.raises(mx.MatrixExtraError, match="Matrix-vector dimensions do not match."):
        X @ mx.dsparseVector([1], [1.0], 4)
    one_col = mx.dgRMatrix([0, 1, 1], [0], [2.0], (2, 1))
    with pytest.raises(mx.MatrixExtraError, match="outer product"):
        one_col @ mx.dsparseVector([1], [1.0], 1)
    with pytest.raises(mx.MatrixExtraError, match="outer product"):
        matmul.matmul(one_col, mx.nsparseVector([1], None, 3))
