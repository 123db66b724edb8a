"""remove_sparse_zeros, filterSparse and check_sparse_matrix (R/utils.R:255-346, :413-489, :582-681).

The argument checks and messages are the reference's R code; the work goes through the device compaction and
validation exports (exports.remove_zero_valued_*, filter_csr / filter_coo, check_valid_*; compact.hip, DESIGN.md
§4.9).  Sparse vectors are reached through the exports only.
"""
from __future__ import annotations

import numpy as np

from . import exports
from .matrices import (MatrixExtraError, RsparseMatrix, TsparseMatrix, check_valid_matrix, dgCMatrix,
                       options, sort_sparse_indices, stop)
from .operators import _as_logical

_SPARSE = (RsparseMatrix, TsparseMatrix, dgCMatrix)
_NO_X = "Method is only applicable for sparse objects with values (slot 'x')."
_COO_SORT = ("Sorting the indices of a TsparseMatrix (sort_coo_indices_*, R/utils.R:22-161) is not on the "
             "accelerated path; call check_sparse_matrix(X, sort=False).")


def _with_slots(X, **slots):
    """X with some slots replaced (R's `attributes(X) <- X_attr`): a new object of X's class, other slots shared."""
    out = type(X).__new__(type(X))
    out.__dict__.update(X.__dict__)
    out.__dict__.update(slots)
    out.Dimnames = list(X.Dimnames)
    return out


def remove_sparse_zeros(X, na_rm=False):
    """R/utils.R:255-346.  Pattern inputs come back as they are; when nothing is removed, X itself (its arrays
    shared) is returned.  The keep rule per class is the reference's: a logical CSR with
    na_rm=True removes only NA and keeps FALSE."""
    if not isinstance(X, _SPARSE):
        stop("Function is only applicable to sparse matrices and sparse vectors.")
    x = getattr(X, "x", None)
    if x is None:                                                             # :268-269
        return X
    logical = x.dtype == np.int32
    if isinstance(X, TsparseMatrix):
        f = exports.remove_zero_valued_coo_logical if logical else exports.remove_zero_valued_coo_numeric
        r = f(X.i, X.j, x, na_rm)
        if r["xx"] is x:
            return X
        return _with_slots(X, i=r["ii"], j=r["jj"], x=r["xx"])
    csc = isinstance(X, dgCMatrix)
    f = exports.remove_zero_valued_csr_logical if logical else exports.remove_zero_valued_csr_numeric
    r = f(X.p, X.i if csc else X.j, x, na_rm)
    if r["values"] is x:
        return X
    if csc:
        return _with_slots(X, p=r["indptr"], i=r["indices"], x=r["values"])
    return _with_slots(X, p=r["indptr"], j=r["indices"], x=r["values"])


def _is_logical_vector(fn):
    """inherits(fn, "logical"): a bool array or list, or an int32 array of R logicals."""
    if isinstance(fn, (list, tuple)):
        fn = np.asarray(fn)
    return isinstance(fn, (np.ndarray, np.bool_)) and np.asarray(fn).dtype in (np.bool_, np.int32)


def filterSparse(X, fn):
    """R/utils.R:582-681 for the CSR / CSC / COO classes: keeps the entries whose `fn(X.x)` is TRUE or NA (an NA
    keeps the entry with NA as its value).  `fn` is a callable on the host, or a bool / R-logical array of nnz
    entries.  A non-logical result goes through as.logical (non-zero TRUE, NaN NA).  A wrong-length result raises
    for a COO too, where R would recycle it."""
    if not isinstance(X, _SPARSE):
        stop("Method is only applicable to sparse matrices and vectors.")
    x = getattr(X, "x", None)
    if _is_logical_vector(fn):                                                # :610-617
        v_orig = np.asarray(fn).reshape(-1)
        if x is None:                                                         # length(X@x): no slot 'x'
            stop(_NO_X)
        if v_orig.size != x.size:
            stop(f"'fn' has incorrect length (expected {x.size}, got {v_orig.size})")
        fn = lambda _x: v_orig                                                # noqa: E731
    if not callable(fn):
        stop("'fn' must be a function.")
    if x is None:
        stop(_NO_X)
    meets = _as_logical(np.asarray(fn(x)).reshape(-1))
    if meets.size != x.size:                                                  # :662-664
        stop(f"'fn' returned incorrect number of entries (expected {x.size}, got {meets.size})")
    meets = np.ascontiguousarray(meets, dtype=np.int32)
    if isinstance(X, TsparseMatrix):
        r = exports.filter_coo(X.i, X.j, x, meets)
        return _with_slots(X, i=r["ii"], j=r["jj"], x=r["xx"])
    if isinstance(X, dgCMatrix):
        r = exports.filter_csr(X.p, X.i, x, meets)
        return _with_slots(X, p=r["indptr"], i=r["indices"], x=r["values"])
    r = exports.filter_csr(X.p, X.j, x, meets)
    return _with_slots(X, p=r["indptr"], j=r["indices"], x=r["values"])


def _sort_csc(X, copy):
    if copy:
        X = dgCMatrix(X.p, X.i.copy(), X.x.copy(), X.Dim, list(X.Dimnames))
    exports.sort_sparse_indices_inplace(X.p, X.i, X.x)
    return X


def check_sparse_matrix(X, sort=True, remove_zeros=True):
    """R/utils.R:439-489: check_valid_matrix, the device index validation (the reference's message of the first
    failing check), remove_sparse_zeros, then the per-row device sort with copy = (nothing was removed).  A CSC is
    checked with its ncol + 1 pointers and its row indices against nrow.  A COO is sorted (the device COO sort,
    DESIGN.md §4.13) only under options["mxgpu.coo_sort_route"]; without it sort=True raises for a TsparseMatrix
    before any device call."""
    if not isinstance(X, _SPARSE):
        stop("Function is only applicable to sparse matrices and sparse vectors.")
    check_valid_matrix(X)
    nrow, ncol = X.Dim
    if isinstance(X, TsparseMatrix):
        if sort and not options.get("mxgpu.coo_sort_route", False):
            stop(_COO_SORT)
        res = exports.check_valid_coo_matrix(X.i, X.j, nrow, ncol)
    elif isinstance(X, RsparseMatrix):
        res = exports.check_valid_csr_matrix(X.p, X.j, nrow, ncol)
    else:
        res = exports.check_valid_csr_matrix(X.p, X.i, ncol, nrow)
    if res:
        raise MatrixExtraError(res["err"])

    def nnz_of(A):
        return A.j.size if isinstance(A, RsparseMatrix) else A.i.size
    nnz_before = nnz_of(X)
    if remove_zeros:
        X = remove_sparse_zeros(X)
    if sort:
        copy = nnz_before == nnz_of(X)
        X = _sort_csc(X, copy) if isinstance(X, dgCMatrix) else sort_sparse_indices(X, copy=copy)
    return X
