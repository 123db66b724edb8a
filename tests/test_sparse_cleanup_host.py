"""remove_sparse_zeros / filterSparse / check_sparse_matrix checks that need no GPU: every argument error raised
before a device call (R/utils.R's messages), the pattern passthrough, the COO sort refusal, and the new C-ABI
entries (declared and exported)."""
import re

import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib

NO_X = "Method is only applicable for sparse objects with values (slot 'x')."


def _csr(cls=mx.dgRMatrix):
    p = np.array([0, 2, 2, 5], np.int32)
    j = np.array([3, 0, 1, 2, 3], np.int32)
    x = {mx.dgRMatrix: np.array([1.5, 0.0, -2.0, 0.0, 4.0]), mx.lgRMatrix: np.array([1, 0, 1, 0, 1], np.int32),
         mx.ngRMatrix: None}[cls]
    return cls(p, j, x, (3, 4))


def _csc():
    return mx.dgCMatrix(np.array([0, 2, 2, 3, 5], np.int32), np.array([2, 0, 1, 0, 2], np.int32),
                        np.array([1.0, 0.0, 3.0, 0.0, 5.0]), (3, 4))


def _coo(cls=mx.dgTMatrix):
    i = np.array([2, 0, 1, 0, 1], np.int32)
    j = np.array([1, 3, 0, 3, 2], np.int32)
    x = {mx.dgTMatrix: np.array([1.5, 0.0, -1.0, 0.5, 0.0]), mx.lgTMatrix: np.array([1, 0, 1, 1, 0], np.int32),
         mx.ngTMatrix: None}[cls]
    return cls(i, j, x, (3, 4))


def test_entry_points_declared_and_exported():
    wanted = {"mx_remove_zero_valued_csr_numeric", "mx_remove_zero_valued_csr_logical",
              "mx_remove_zero_valued_coo_numeric", "mx_remove_zero_valued_coo_logical",
              "mx_remove_zero_valued_svec_numeric", "mx_remove_zero_valued_svec_integer",
              "mx_remove_zero_valued_svec_logical", "mx_check_valid_csr_matrix", "mx_check_valid_coo_matrix",
              "mx_check_valid_svec", "mx_rebuild_indptr_after_filter", "mx_filter_sparse_begin",
              "mxd_compact_workspace_bytes", "mxd_compact_count", "mxd_compact_fill", "mxd_validate_indices"}
    assert wanted <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in wanted)


def test_compact_workspace_grows_with_entries():
    lib = _lib.load()
    assert 0 < lib.mxd_compact_workspace_bytes(1000) < lib.mxd_compact_workspace_bytes(1 << 24)


@pytest.mark.parametrize("X", [_csr(mx.ngRMatrix), _coo(mx.ngTMatrix)])
@pytest.mark.parametrize("na_rm", [False, True])
def test_remove_sparse_zeros_returns_pattern_inputs(X, na_rm):
    assert mx.remove_sparse_zeros(X, na_rm) is X                    # R/utils.R:268-269


@pytest.mark.parametrize("fn", [mx.remove_sparse_zeros, mx.check_sparse_matrix])
def test_non_sparse_inputs_are_refused(fn):
    with pytest.raises(mx.MatrixExtraError, match="Function is only applicable to sparse matrices and sparse vectors."):
        fn(np.ones((2, 2)))
    with pytest.raises(mx.MatrixExtraError, match="Method is only applicable to sparse matrices and vectors."):
        mx.filterSparse(np.ones((2, 2)), lambda x: x > 0)


@pytest.mark.parametrize("X", [_csr(), _csr(mx.lgRMatrix), _csc(), _coo(), _coo(mx.lgTMatrix)])
@pytest.mark.parametrize("mask", [np.ones(4, bool), np.ones(6, np.int32), [True, False]])
def test_filter_logical_vector_of_wrong_length(X, mask):
    n = np.asarray(mask).size
    with pytest.raises(mx.MatrixExtraError, match=re.escape(f"'fn' has incorrect length (expected 5, got {n})")):
        mx.filterSparse(X, mask)                                    # R/utils.R:612-614


@pytest.mark.parametrize("X", [_csr(), _csc(), _coo(), _coo(mx.lgTMatrix)])
def test_filter_function_result_of_wrong_length(X):
    # CSR / CSC: R/utils.R:662-664; a COO raises the same error where R would recycle
    with pytest.raises(mx.MatrixExtraError,
                       match=re.escape("'fn' returned incorrect number of entries (expected 5, got 3)")):
        mx.filterSparse(X, lambda x: np.ones(3, bool))


@pytest.mark.parametrize("fn", [3.0, "x > 0", np.ones(5), None])
def test_filter_fn_must_be_a_function(fn):
    with pytest.raises(mx.MatrixExtraError, match=re.escape("'fn' must be a function.")):
        mx.filterSparse(_csr(), fn)


@pytest.mark.parametrize("X", [_csr(mx.ngRMatrix), _coo(mx.ngTMatrix)])
@pytest.mark.parametrize("fn", [lambda x: x, np.ones(5, bool)])
def test_filter_pattern_inputs_are_refused(X, fn):
    with pytest.raises(mx.MatrixExtraError, match=re.escape(NO_X)):
        mx.filterSparse(X, fn)


@pytest.mark.parametrize("cls", [mx.dgTMatrix, mx.lgTMatrix, mx.ngTMatrix])
def test_check_sparse_matrix_refuses_to_sort_a_coo(cls):
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        mx.check_sparse_matrix(_coo(cls))
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        mx.check_sparse_matrix(_coo(cls), sort=True, remove_zeros=False)


def test_check_sparse_matrix_runs_check_valid_matrix_first():
    T = _coo()
    T.j = T.j[:-1]
    with pytest.raises(mx.MatrixExtraError, match="row and column indices have different length"):
        mx.check_sparse_matrix(T)
    X = _csr()
    X.p = np.array([0, 2, 5], np.int32)
    with pytest.raises(mx.MatrixExtraError, match="'p' doesn't match with dimension"):
        mx.check_sparse_matrix(X)
