"""Host-side mirror of R/assignment.R: `X[i, j] <- value` for a dgRMatrix.

`assign_csr(x, i, j, value)` takes R-style selectors (1-based integers, negative = exclusion, logical masks, names;
`None` = missing) and returns a NEW dgRMatrix; `x` is never changed.  Branch order and messages are
assign_csr_internal's (R/assignment.R:37-513).  What is on the device:

    scalar value (a one-element vector is a scalar)      -> the twenty set_*_to_zero / set_*_to_const exports
    sparse matrix of whole rows, all columns selected    -> set_rowseq_to_smat / set_arbitrary_rows_to_smat

`x[, ] <- 0` and `x[, ] <- value` never reach native code in the reference either and are done here.  Every route
the reference sends through the `Matrix` package (assign_through_matrix) or through its vector-valued routines
(set_single_row_to_rowvec, set_single_col_to_colvec, set_single_*_to_svec) raises MatrixExtraError naming the route:
there is no silent fallback.

Under options["mxgpu.assign_vec_route"] (off unless set) the four vector-valued routines run on the
device instead of refusing: one row with all columns, or all rows with one column, given a dense vector, a
sparseVector, or a sparse matrix of one row or one column (which becomes the sparseVector it spells).  Everything
else refuses as without the option.

Rows of `x` that are not sorted: a sorted copy is made first (sort_sparse_indices(copy=True)), so the result differs
from the reference's only in the order inside rows the assignment does not touch; the reference instead sorts the
selected rows of the caller's own vectors in place, which is not done here.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import exports
from .matrices import (DenseMatrix, MatrixExtraError, NA_INTEGER, NA_REAL, RsparseMatrix, TsparseMatrix,
                       as_csr_matrix, as_sparse_vector, dgCMatrix, dgRMatrix, dsparseVector, float32, nsparseVector,
                       options, sort_sparse_indices, sparseVector, stop)
from .slice import get_ij_properties

_SPARSE_MATRIX = (RsparseMatrix, TsparseMatrix, dgCMatrix)


def throw_shape_err():
    stop("Values to assign do not match with matrix dimensions.")


def _not_on_device(route):
    raise MatrixExtraError(f"This assignment takes the reference's route '{route}', which is not on the device.")


def _vec_route():
    return bool(options.get("mxgpu.assign_vec_route", False))


def check_shapes_are_assignable_2d(x1, x2, y1, y2):
    """src/assignment.cpp:2604-2617."""
    return y1 * y2 != 0 and not (y1 * y2 > x1 * x2 or (x1 * x2) % (y1 * y2) != 0)


def check_shapes_are_assignable_1d(x1, x2, vlen):
    """src/assignment.cpp:2624-2637."""
    return vlen != 0 and not (vlen > x1 * x2 or (x1 * x2) % vlen != 0)


def check_shapes_are_assignable_1d_v2(xlen, y1, y2):
    """src/assignment.cpp:2639-2647."""
    return y1 * y2 != 0 and not (y1 * y2 > xlen or xlen % (y1 * y2) != 0)


def _has_na(idx):
    if idx is None:
        return False
    a = np.asarray(idx)
    if a.dtype.kind == "f":
        return bool(np.isnan(a).any())
    if a.dtype.kind == "i":
        return bool((a == NA_INTEGER).any())
    if a.dtype.kind == "O":
        return any(v is None for v in a.reshape(-1).tolist())
    return False


def _as_f64(a):
    """as.numeric() of a numeric / integer / logical array: integer and logical NA become NA_real_."""
    a = np.asarray(a)
    if a.dtype == np.int32:
        return np.where(a == NA_INTEGER, NA_REAL, a.astype(np.float64))
    return a.astype(np.float64)


def _nrow_of(value):
    """NROW(value), or None for a value `[<-` is not registered for (R/assignment.R:39-44)."""
    if isinstance(value, (bool, int, float, np.bool_, np.integer, np.floating)):
        return 1
    if isinstance(value, np.ndarray) and value.dtype.kind in "biuf" and value.ndim in (1, 2):
        return value.shape[0]
    if isinstance(value, float32):
        return value.Data.shape[0]
    if isinstance(value, sparseVector):
        return len(value)
    if isinstance(value, _SPARSE_MATRIX):
        return value.Dim[0]
    return None


def _n_entries(value):
    """Stored entries of a sparse value (the @x / @i / @j length tests of R/assignment.R:79-84)."""
    if isinstance(value, sparseVector):
        return value.i.size
    if isinstance(value, TsparseMatrix):
        return value.i.size
    if isinstance(value, dgCMatrix):
        return value.i.size
    return value.j.size


def _sorted_operand(x):
    if exports.rows_are_sorted(x.p, x.j):
        return x
    return sort_sparse_indices(x, copy=True)


def _numeric_svec(value, route):
    """The sparseVector with float64 @x (integer and logical NA become NA_real_).  An nsparseVector has no @x for the
    reference to read (R/assignment.R:320, :340) and is refused."""
    if isinstance(value, nsparseVector):
        _not_on_device(f"{route} (nsparseVector value, which has no @x)")
    return value if isinstance(value, dsparseVector) else as_sparse_vector(value)


def _spelled_vector(value):
    """The sparseVector a sparse matrix of one row or one column spells.  The reference hands the matrix's own index
    and value slots to set_single_*_to_svec (R/assignment.R:386, :399, :461, :474), with ncol(value) as the length:
    for a one-column value that length is 1, a defect.  Here the length is the vector's, and a column assignment
    sorts the vector like any other sparseVector."""
    return as_sparse_vector(value)


def _finish(x, res):
    """attributes(x) with p / j / x replaced (R/assignment.R:507-512): a new object, dimnames kept."""
    return dgRMatrix(res["indptr"], res["indices"], res["values"], x.Dim, list(x.Dimnames))


def assign_csr(x, i=None, j=None, value=None):
    """`x[i, j] <- value` (R/assignment.R:515-519); returns the new matrix (a DenseMatrix for `x[, ] <- const`)."""
    if not isinstance(x, dgRMatrix):
        stop("'[<-' is only registered for dgRMatrix (R/assignment.R:521-553).")
    return _assign_csr_internal(x, i, j, value, None)


def _assign_csr_internal(x, i, j, value, P):
    E = exports
    nrow_v = None if value is None else _nrow_of(value)
    if not nrow_v:                                               # R/assignment.R:39-44
        stop("Invalid value to assign.")
    if isinstance(value, float32):                               # float::dbl()
        value = value.Data.astype(np.float64)
    if isinstance(value, np.ndarray):
        value = _as_f64(value.reshape(-1, order="F"))            # as.numeric(matrix): column-major
    elif isinstance(value, (bool, int, float, np.bool_, np.integer, np.floating)):
        value = _as_f64(np.array([value], dtype=np.int32 if isinstance(value, np.int32) else None))

    if P is None:
        if _has_na(i) or _has_na(j):                             # :56-57
            stop("Indices contain NAs.")
        P = get_ij_properties(x, i, j)
    i, j = P.i, P.j
    all_i, all_j = P.all_i, P.all_j
    i_seq = P.i_is_seq or P.i_is_rev_seq
    j_seq = P.j_is_seq or P.j_is_rev_seq
    nrow, ncol = x.Dim

    if np.unique(i).size != i.size or np.unique(j).size != j.size:      # :70-77
        _not_on_device("assign_through_matrix (duplicated indices)")
    if i.size == 0 or j.size == 0:                               # nothing is selected
        return _finish(x, dict(indptr=x.p, indices=x.j, values=x.x))

    if isinstance(value, (sparseVector,) + _SPARSE_MATRIX) and _n_entries(value) == 0:     # :79-95
        if isinstance(value, sparseVector):
            if not check_shapes_are_assignable_1d(i.size, j.size, len(value)):
                throw_shape_err()
        elif not check_shapes_are_assignable_2d(i.size, j.size, value.Dim[0], value.Dim[1]):
            throw_shape_err()
        value = np.zeros(1)

    if isinstance(value, np.ndarray) and value.size == 1:        # :119-247
        v = float(value[0])
        rows0, cols0 = (i - 1).astype(np.int32), (j - 1).astype(np.int32)
        if v == 0:                                               # !is.na(value) && value == 0
            if all_i and all_j:                                  # :123-130
                return dgRMatrix(np.zeros(nrow + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), x.Dim,
                                 list(x.Dimnames))
            x = _sorted_operand(x)
            a = (x.p, x.j, x.x)
            if all_j:
                if i.size == 1:
                    res = E.set_single_row_to_zero(*a, int(rows0[0]))
                elif i_seq:
                    res = E.set_rowseq_to_zero(*a, int(rows0.min()), int(rows0.max()))
                else:
                    res = E.set_arbitrary_rows_to_zero(*a, rows0)
            elif all_i:
                if j.size == 1:
                    res = E.set_single_col_to_zero(*a, int(cols0[0]))
                elif j_seq:
                    res = E.set_colseq_to_zero(*a, int(cols0.min()), int(cols0.max()), ncol)
                else:
                    res = E.set_arbitrary_cols_to_zero(*a, cols0, ncol)
            elif i.size == 1 and j.size == 1:
                res = E.set_single_val_to_zero(*a, int(rows0[0]), int(cols0[0]))
            elif j.size == 1:
                res = E.set_arbitrary_rows_single_col_to_zero(*a, rows0, int(cols0[0]), ncol)
            elif i.size == 1:
                res = E.set_single_row_arbitrary_cols_to_zero(*a, int(rows0[0]), cols0, ncol)
            else:
                res = E.set_arbitrary_rows_arbitrary_cols_to_zero(*a, rows0, cols0, ncol)
            return _finish(x, res)

        if all_i and all_j:                                      # :187-195
            warnings.warn("Warning: attempting to set all coordinates in a sparse matrix.")
            return DenseMatrix(np.full(x.Dim, v, dtype=np.float64, order="F"), list(x.Dimnames))
        x = _sorted_operand(x)
        a = (x.p, x.j, x.x)
        if all_j:
            if i.size == 1:
                res = E.set_single_row_to_const(*a, ncol, int(rows0[0]), v)
            elif i_seq:
                res = E.set_rowseq_to_const(*a, int(rows0.min()), int(rows0.max()), ncol, v)
            else:
                res = E.set_arbitrary_rows_to_const(*a, rows0, ncol, v)
        elif all_i:
            if j.size == 1:
                res = E.set_single_col_to_const(*a, ncol, int(cols0[0]), v)
            elif j_seq:
                res = E.set_colseq_to_const(*a, int(cols0.min()), int(cols0.max()), ncol, v)
            else:
                res = E.set_arbitrary_cols_to_const(*a, cols0, ncol, v)
        elif i.size == 1 and j.size == 1:
            res = E.set_single_val_to_const(*a, ncol, int(rows0[0]), int(cols0[0]), v)
        elif j.size == 1:
            res = E.set_arbitrary_rows_single_col_to_const(*a, rows0, int(cols0[0]), v, ncol)
        elif i.size == 1:
            res = E.set_single_row_arbitrary_cols_to_const(*a, int(rows0[0]), cols0, ncol, v)
        else:
            res = E.set_arbitrary_rows_arbitrary_cols_to_const(*a, rows0, cols0, ncol, v)
        return _finish(x, res)

    if isinstance(value, np.ndarray):                            # a vector longer than one, :249-299
        n = value.size
        if all_i and all_j:
            if not check_shapes_are_assignable_1d(nrow, ncol, n):
                throw_shape_err()
            _not_on_device("x[, ] <- vector")
        if all_j and i.size == 1:
            if n > ncol or ncol % n != 0:
                throw_shape_err()
            if not _vec_route():
                _not_on_device("set_single_row_to_rowvec")
            return _finish(x, E.set_single_row_to_rowvec(x.p, x.j, x.x, ncol, int(i[0]) - 1, value))
        if all_i and j.size == 1 and not all_j:
            if n > nrow or nrow % n != 0:
                throw_shape_err()
            if not _vec_route():
                _not_on_device("set_single_col_to_colvec")
            x = _sorted_operand(x)                               # an insert lands at its ascending place
            return _finish(x, E.set_single_col_to_colvec(x.p, x.j, x.x, ncol, int(j[0]) - 1, value))
        if not all_i and not all_j and not check_shapes_are_assignable_1d(i.size, j.size, n):
            throw_shape_err()
        _not_on_device("assign_through_matrix (vector value)")

    if isinstance(value, sparseVector):                          # :301-351
        if len(value) == 1:                                      # as.numeric(value)
            one = 1.0 if value.x is None else float(_as_f64(value.x)[0])
            return _assign_csr_internal(x, i, j, one, P)
        if all_j and not all_i and i.size == 1:
            if len(value) > ncol or ncol % len(value) != 0:
                throw_shape_err()
            if not _vec_route():
                _not_on_device("set_single_row_to_svec")
            value = _numeric_svec(value, "set_single_row_to_svec")
            return _finish(x, E.set_single_row_to_svec(x.p, x.j, x.x, ncol, int(i[0]) - 1, value.i - 1, value.x,
                                                       len(value)))                # ii as stored (:320)
        if all_i and not all_j and j.size == 1:
            if len(value) > nrow or nrow % len(value) != 0:
                throw_shape_err()
            if not _vec_route():
                _not_on_device("set_single_col_to_svec")
            value = sort_sparse_indices(_numeric_svec(value, "set_single_col_to_svec"), copy=True)     # :335-338
            x = _sorted_operand(x)
            return _finish(x, E.set_single_col_to_svec(x.p, x.j, x.x, ncol, int(j[0]) - 1, value.i - 1, value.x,
                                                       len(value)))
        if all_i and all_j and not check_shapes_are_assignable_1d(nrow, ncol, len(value)):
            throw_shape_err()
        _not_on_device("assign_through_matrix (sparseVector value)")

    # a sparse matrix with entries, :353-494
    v_nrow, v_ncol = value.Dim
    if all_i and all_j:
        if not check_shapes_are_assignable_2d(nrow, ncol, v_nrow, v_ncol):
            throw_shape_err()
        if (nrow, ncol) == (v_nrow, v_ncol):                     # :361-362
            return as_csr_matrix(value)
        _not_on_device("assign_through_matrix (sparse matrix recycled as a sparseVector)")
    if all_j:
        if i.size == 1:
            if not check_shapes_are_assignable_1d_v2(ncol, v_nrow, v_ncol):
                throw_shape_err()
            if v_nrow == 1 and v_ncol == 1:                      # :375-378
                return _assign_csr_internal(x, i, j, as_csr_matrix(value).toarray().reshape(-1), P)
            if _vec_route() and (v_nrow == 1 or v_ncol == 1):
                return _assign_csr_internal(x, i, j, _spelled_vector(value), P)
            _not_on_device("set_single_row_to_svec")
        if v_nrow != i.size or v_ncol != ncol:
            if i_seq:                                            # :422-425
                _not_on_device("assign_through_matrix (sparse matrix that is not whole rows)")
            throw_shape_err()            # the reference's arbitrary branch (:428-439) reads past such a value
        V = as_csr_matrix(value)                                 # R / T / C sparse values; rows go in as stored
        rows0 = (i - 1).astype(np.int32)
        if i.size == nrow and not i_seq:                         # :430-431: value[order(i), ], the gather alone
            res = E.copy_csr_rows_numeric(V.p, V.j, V.x, np.argsort(i, kind="stable").astype(np.int32))
        elif P.i_is_seq:                                         # :411-420
            res = E.set_rowseq_to_smat(x.p, x.j, x.x, int(rows0[0]), int(rows0[-1]), V.p, V.j, V.x)
        else:
            # rev-seq and arbitrary selectors alike: the device takes the selector in the caller's order, so the
            # reference's value[order(i), ] re-gather on the host (:417-418, :432-436) is not needed
            res = E.set_arbitrary_rows_to_smat(x.p, x.j, x.x, rows0, V.p, V.j, V.x)
        return _finish(x, res)
    if all_i and j.size == 1:
        if not check_shapes_are_assignable_1d_v2(nrow, v_nrow, v_ncol):
            throw_shape_err()
        if v_nrow == 1 and v_ncol == 1:
            return _assign_csr_internal(x, i, j, as_csr_matrix(value).toarray().reshape(-1), P)
        if _vec_route() and (v_nrow == 1 or v_ncol == 1):
            return _assign_csr_internal(x, i, j, _spelled_vector(value), P)
        _not_on_device("set_single_col_to_svec")
    _not_on_device("assign_through_matrix (sparse matrix value)")
