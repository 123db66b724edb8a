"""The mirror of the transposed products on the GPU (matmul.py over exports.csr_tmatvec / csr_tmatmul_dense): every
signature that used to end in "Unsupported operand types", against dense numpy on the reference's operator fixture
shape (a 100 x 35 matrix of density 0.4, tests/testthat/test-matmul.R) with n = 20.  General floats are compared at the
tolerances of tests/test_gpu_host_mirror.py (rtol 1e-10, atol 1e-12); integer-valued, logical and pattern data are
compared exactly: every product and every partial sum is an integer f64 holds, whatever the order."""
import numpy as np
import pytest

import matrixextra_amd as mx
from conftest import csr_to_dense, rand_csr

pytestmark = pytest.mark.gpu

M, K, N = 100, 35, 20
ROWN, COLN = ["r%d" % i for i in range(M)], ["c%d" % i for i in range(K)]
TOL = dict(rtol=1e-10, atol=1e-12)
NA = mx.NA_INTEGER


def dense(rows, cols, seed, names=None):
    Y = np.round(np.random.default_rng(seed).normal(size=(rows, cols)), 2)
    return mx.DenseMatrix(Y, names)


def csr_X(integer=False):
    p, j, x = rand_csr(M, K, 0.4, 51, sorted_cols=False)
    if integer:
        x = np.random.default_rng(52).integers(1, 10, size=j.size).astype(np.float64)
    return mx.dgRMatrix(p, j, x, (M, K), [ROWN, COLN]), csr_to_dense(p, j, x, K)


def csc_X():
    """an M x K dgCMatrix: its arrays are the CSR of the K x M transpose"""
    p, i, x = rand_csr(K, M, 0.4, 53, sorted_cols=False)
    return mx.dgCMatrix(p, i, x, (M, K), [ROWN, COLN]), csr_to_dense(p, i, x, M).T


def test_crossprod_of_a_csr(gpu):
    X, D = csr_X()
    Y = dense(M, N, 1, [["y%d" % i for i in range(M)], ["z%d" % i for i in range(N)]])
    got = mx.crossprod(X, Y)
    assert isinstance(got, mx.DenseMatrix) and got.shape == (K, N) and got.Dimnames == [COLN, Y.Dimnames[1]]
    np.testing.assert_allclose(np.asarray(got), D.T @ np.asarray(Y), **TOL)
    v = np.round(np.random.default_rng(2).normal(size=M), 2)
    got = mx.crossprod(X, v)
    assert got.shape == (K, 1) and got.Dimnames == [COLN, None]
    np.testing.assert_allclose(np.asarray(got)[:, 0], D.T @ v, **TOL)
    with pytest.raises(mx.MatrixExtraError, match="Matrix-vector dimensions do not match."):
        mx.crossprod(X, np.ones(K))
    with pytest.raises(mx.MatrixExtraError, match="Matrix dimensions do not match."):
        mx.crossprod(X, np.ones((K, 2)))


def test_dense_times_a_csr(gpu):
    X, D = csr_X()
    v = np.round(np.random.default_rng(3).normal(size=M), 2)
    got = v @ X
    assert isinstance(got, mx.DenseMatrix) and got.shape == (1, K) and got.Dimnames == [None, COLN]
    np.testing.assert_allclose(np.asarray(got)[0], v @ D, **TOL)
    Y = dense(N, M, 4, [["y%d" % i for i in range(N)], None])
    got = Y @ X
    assert got.shape == (N, K) and got.flags.f_contiguous and got.Dimnames == [Y.Dimnames[0], COLN]
    np.testing.assert_allclose(np.asarray(got), np.asarray(Y) @ D, **TOL)
    got = np.ascontiguousarray(np.asarray(Y)) @ X                        # a row-major matrix on the left
    np.testing.assert_allclose(np.asarray(got), np.asarray(Y) @ D, **TOL)


def test_a_csc_on_the_left_and_under_tcrossprod(gpu):
    X, D = csc_X()
    Y = dense(K, N, 5, [None, ["z%d" % i for i in range(N)]])
    got = X @ Y
    assert got.shape == (M, N) and got.Dimnames == [ROWN, Y.Dimnames[1]]
    np.testing.assert_allclose(np.asarray(got), D @ np.asarray(Y), **TOL)
    v = np.round(np.random.default_rng(6).normal(size=K), 2)
    got = X @ v
    assert got.shape == (M, 1) and got.Dimnames == [ROWN, None]
    np.testing.assert_allclose(np.asarray(got)[:, 0], D @ v, **TOL)
    Z = dense(N, K, 7, [["y%d" % i for i in range(N)], None])
    got = mx.tcrossprod(Z, X)
    assert got.shape == (N, M) and got.flags.f_contiguous and got.Dimnames == [Z.Dimnames[0], ROWN]
    np.testing.assert_allclose(np.asarray(got), np.asarray(Z) @ D.T, **TOL)


def upper(n, seed):
    """(p, j, x, dense) of a random upper triangle with a full diagonal, integer-valued"""
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((n, n)) < 0.3) | np.eye(n, dtype=bool)
    U = np.where(mask, rng.integers(1, 9, (n, n)).astype(np.float64), 0.0)
    r, c = np.nonzero(mask)
    p = np.zeros(n + 1, dtype=np.int32)
    p[1:] = np.cumsum(mask.sum(axis=1))
    return p, c.astype(np.int32), U[r, c], U


def test_symmetric_and_triangular_operands_are_expanded(gpu):
    p, j, x, U = upper(K, 8)
    S = mx.dsRMatrix(p, j, x, (K, K), [None, COLN], uplo="U")
    full = U + np.triu(U, 1).T
    Y = np.random.default_rng(9).integers(-4, 5, size=(K, N)).astype(np.float64)
    got = mx.crossprod(S, Y)
    assert got.shape == (K, N) and np.array_equal(np.asarray(got), full.T @ Y)
    v = np.arange(1.0, K + 1)
    assert np.array_equal(np.asarray(v @ S)[0], v @ full)
    # the same slots read as a CSC hold the lower triangle t(U)
    T = mx.dtCMatrix(p, j, x, (K, K), [None, COLN], uplo="L", diag="N")
    got = T @ Y
    assert got.shape == (K, N) and np.array_equal(np.asarray(got), U.T @ Y)
    assert np.array_equal(np.asarray(T @ v)[:, 0], U.T @ v)
    assert np.array_equal(np.asarray(mx.tcrossprod(Y.T.copy(), T)), Y.T @ U)


def test_logical_and_pattern_matrices_and_na_in_the_dense_operand(gpu):
    p, j, xl = rand_csr(M, K, 0.4, 54, sorted_cols=False, dtype="l")
    rows = np.repeat(np.arange(M), np.diff(p))
    xl[(xl == NA) & (rows > 2)] = 1                                     # NAs in the first three rows only
    v = np.random.default_rng(10).integers(-4, 5, size=M).astype(np.float64)
    with np.errstate(invalid="ignore"):
        want = np.zeros(K)
        np.add.at(want, j, np.where(xl == NA, np.nan, xl.astype(np.float64)) * v[rows])
    got = np.asarray(mx.crossprod(mx.lgRMatrix(p, j, xl, (M, K)), v))[:, 0]
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(got, want, equal_nan=True)
    counts = np.zeros(K)
    np.add.at(counts, j, v[rows])
    N_ = mx.ngRMatrix(p, j, None, (M, K))
    assert np.array_equal(np.asarray(mx.crossprod(N_, v))[:, 0], counts)
    assert np.array_equal(np.asarray(v @ N_)[0], counts)
    # an integer vector with NA: NA_real_ reaches only the columns that store an entry in its rows
    X, D = csr_X(integer=True)
    vi = np.random.default_rng(11).integers(-4, 5, size=M).astype(np.int32)
    vi[[3, 40]] = NA
    hit = (D[3] != 0) | (D[40] != 0)
    assert hit.any() and not hit.all()
    got = np.asarray(mx.crossprod(X, vi))[:, 0]
    vf = np.where(vi == NA, 0.0, vi.astype(np.float64))
    assert np.array_equal(np.isnan(got), hit) and np.array_equal(got[~hit], (D.T @ vf)[~hit])
    Yi = np.random.default_rng(12).integers(-4, 5, size=(M, 3)).astype(np.int32)
    Yi[3, 1] = NA
    got = np.asarray(mx.crossprod(X, Yi))
    assert np.array_equal(np.isnan(got[:, 1]), D[3] != 0) and not np.isnan(got[:, [0, 2]]).any()
    assert np.array_equal(got[:, 0], D.T @ Yi[:, 0].astype(np.float64))


def test_the_gradient_is_colmeans_of_the_product_bit_for_bit(gpu):
    """crossprod(X, r) / nrow against colMeans(X * r) (vignettes/Introducing_MatrixExtra.Rmd:454-470), integer-valued"""
    X, D = csr_X(integer=True)
    r = np.random.default_rng(13).integers(-9, 10, size=M).astype(np.float64)
    grad = np.asarray(mx.crossprod(X, r))[:, 0] / M
    means = np.asarray(mx.colMeans(X * r))
    assert np.array_equal(grad.view(np.uint64), means.view(np.uint64))
    assert np.array_equal(grad, (D.T @ r) / M)
