"""Host-side mirror of R/matmul.R for the <CSR, dense> products (the north-star path).

Function names, argument meaning, checks, error messages and result shapes
follow the reference's R glue; the numerics happen in the HIP kernels behind
matrixextra_amd.exports.  Reference call stacks: SURVEY.md §3.1-3.2.
"""
from __future__ import annotations

import numpy as np

from . import exports
from .matrices import (NA_INTEGER, NA_REAL, DenseMatrix, RsparseMatrix, as_csc_matrix, as_csr_matrix, as_sparse_vector,
                       check_valid_matrix, dgCMatrix, dgRMatrix, dimnames_of, dsparseVector, float32, isparseVector,
                       lgRMatrix, lsparseVector, ngRMatrix, nsparseVector, options, sort_sparse_indices, sparseVector, stop)


def _nthreads():
    return max(int(options.get("MatrixExtra.nthreads", 1)), 1)


def _nrow(x):
    return x.Dim[0] if hasattr(x, "Dim") else (x.Data.shape[0] if isinstance(x, float32) else x.shape[0])


def _ncol(x):
    return x.Dim[1] if hasattr(x, "Dim") else (x.Data.shape[1] if isinstance(x, float32) else x.shape[1])


def check_dimensions_match(x, y, matmult=False, crossprod=False, tcrossprod=False):
    """R/matmul.R:130-146."""
    if matmult:
        inner_x, inner_y = _ncol(x), _nrow(y)
    elif crossprod:
        inner_x, inner_y = _nrow(x), _nrow(y)
    elif tcrossprod:
        inner_x, inner_y = _ncol(x), _ncol(y)
    else:
        stop("Unexpected error. Please open an issue in GitHub explaining what you were doing.")
    if inner_x != inner_y:
        stop("Matrix dimensions do not match.")


def _product_dimnames(x, y, matmult=False, crossprod=False):
    """row names of op(x), column names of op(y) — R/matmul.R:148-167"""
    dx, dy = dimnames_of(x), dimnames_of(y)
    if matmult:
        return dx[0], dy[1]
    if crossprod:
        return dx[1], dy[1]
    return dx[0], dy[0]


def set_dimnames(res, x, y, matmult=False, crossprod=False, tcrossprod=False):
    """R/matmul.R:148-167."""
    rnames, cnames = _product_dimnames(x, y, matmult, crossprod)
    if isinstance(res, float32):
        res.Dimnames = [rnames, cnames]
        return res
    return DenseMatrix(res, [rnames, cnames])


def _as_double_matrix(y):
    y = np.asarray(y)
    if y.ndim != 2:
        stop("Matrix dimensions do not match.")
    return y if y.dtype == np.float64 else y.astype(np.float64)      # mode(y) <- "double"  R/matmul.R:443


# ---- CSR x dense ---------------------------------------------------------------------------------
def tcrossprod_csr_dense(x, y):
    """tcrossprod(RsparseMatrix, matrix) — R/matmul.R:436-457."""
    check_dimensions_match(x, y, tcrossprod=True)
    nthreads = _nthreads()
    y_names = dimnames_of(y)
    yd = _as_double_matrix(y)
    x = as_csr_matrix(x)
    check_valid_matrix(x)
    res = exports.tcrossprod_csr_dense_numeric(x.p, x.j, x.x, yd, nthreads)
    return set_dimnames(res, x, DenseMatrix(yd, y_names), tcrossprod=True)


def gemm_csr_dense(x, y):
    """RsparseMatrix %*% matrix = tcrossprod_csr_dense(x, t(y)) — R/matmul.R:463-465."""
    y_names = dimnames_of(y)
    yt = DenseMatrix(np.asarray(y).T, [y_names[1], y_names[0]])      # base-R t(y): a dense transpose
    return tcrossprod_csr_dense(x, yt)


def tcrossprod_csr_f32(x, y):
    """tcrossprod(RsparseMatrix, float32) — R/matmul.R:514-536."""
    check_dimensions_match(x, y, tcrossprod=True)
    nthreads = _nthreads()
    x = as_csr_matrix(x)
    check_valid_matrix(x)
    res = float32(exports.tcrossprod_csr_dense_float32(x.p, x.j, x.x, y.Data, nthreads))
    return set_dimnames(res, x, y, tcrossprod=True)


def gemm_csr_f32(x, y):
    """RsparseMatrix %*% float32 — R/matmul.R:471-512 (transposes y with float's t())."""
    yt = float32(y.Data.T, [dimnames_of(y)[1], dimnames_of(y)[0]])
    return tcrossprod_csr_f32(x, yt)


# ---- dense x CSC / dense x t(CSR) ----------------------------------------------------------------
def gemm_dense_csc(x, y):
    """matrix %*% CsparseMatrix — R/matmul.R:171-198."""
    check_dimensions_match(x, y, matmult=True)
    nthreads = _nthreads()
    x_names = dimnames_of(x)
    xd = _as_double_matrix(x)
    check_valid_matrix(y)
    res = exports.matmul_dense_csc_numeric(xd, y.p, y.i, y.x, nthreads)
    return set_dimnames(res, DenseMatrix(xd, x_names), y, matmult=True)


def gemm_f32_csc(x, y):
    """float32 %*% CsparseMatrix — R/matmul.R:202-279."""
    check_dimensions_match(x, y, matmult=True)
    check_valid_matrix(y)
    res = float32(exports.matmul_dense_csc_float32(x.Data, y.p, y.i, y.x, _nthreads()))
    return set_dimnames(res, x, y, matmult=True)


def crossprod_dense_csc(x, y):
    """crossprod(matrix, CsparseMatrix) = gemm_dense_csc(t(x), y) — R/matmul.R:387-391."""
    x_names = dimnames_of(x)
    return gemm_dense_csc(DenseMatrix(np.asarray(x).T, [x_names[1], x_names[0]]), y)


def tcrossprod_dense_csr(x, y):
    """tcrossprod(matrix, RsparseMatrix) — R/matmul.R:283-305."""
    check_dimensions_match(x, y, tcrossprod=True)
    nthreads = _nthreads()
    x_names = dimnames_of(x)
    xd = _as_double_matrix(x)
    y = as_csr_matrix(y)
    check_valid_matrix(y)
    res = exports.tcrossprod_dense_csr_numeric(xd, y.p, y.j, y.x, nthreads, y.Dim[1])
    return set_dimnames(res, DenseMatrix(xd, x_names), y, tcrossprod=True)


def tcrossprod_f32_csr(x, y):
    """tcrossprod(float32, RsparseMatrix) — R/matmul.R:309-383."""
    check_dimensions_match(x, y, tcrossprod=True)
    y = as_csr_matrix(y)
    check_valid_matrix(y)
    res = float32(exports.tcrossprod_dense_csr_float32(x.Data, y.p, y.j, y.x, _nthreads(), y.Dim[1]))
    return set_dimnames(res, x, y, tcrossprod=True)


# ---- CSR x dense vector ------------------------------------------------------------------------------
def gemv_csr_vec(x, y):
    """RsparseMatrix %*% numeric/integer/logical/float32 vector or sparseVector — R/matmul.R:545-657.
    Returns an (nrow, 1) matrix like `matrix(res, ncol=1)`; float32 input -> float32 result."""
    if isinstance(y, sparseVector):
        return _gemv_csr_svec(x, y)
    is_f32 = isinstance(y, float32)
    yv = y.Data.reshape(-1) if is_f32 else np.asarray(y)
    if yv.ndim != 1:
        stop("Matrix-vector dimensions do not match.")
    if x.Dim[1] != yv.size:
        stop("Matrix-vector dimensions do not match.")
    nthreads = options.get("MatrixExtra.nthreads", 1)
    check_valid_matrix(x)
    x = as_csr_matrix(x)
    if is_f32:
        res = exports.matmul_csr_dvec_float32(x.p, x.j, x.x, yv, nthreads)
    elif yv.dtype == np.float64:
        res = exports.matmul_csr_dvec_numeric(x.p, x.j, x.x, yv, nthreads)
    elif yv.dtype == np.bool_:
        res = exports.matmul_csr_dvec_logical(x.p, x.j, x.x, yv.astype(np.int32), nthreads)
    elif yv.dtype == np.int32:
        # R keeps integer and logical apart by type; an int32 vector is an R integer unless tagged
        if getattr(y, "r_logical", False):
            res = exports.matmul_csr_dvec_logical(x.p, x.j, x.x, yv, nthreads)
        else:
            res = exports.matmul_csr_dvec_integer(x.p, x.j, x.x, yv, nthreads)
    else:
        return gemv_csr_vec(x, yv.astype(np.float64))        # as.numeric(y) fallback, R/matmul.R:589-593
    rn = dimnames_of(x)[0]
    if is_f32:
        return float32(res.reshape(-1, 1), [rn, None])
    return DenseMatrix(res.reshape(-1, 1), [rn, None])


_SVEC_OUTER = ("A one-column RsparseMatrix times a sparseVector is the reference's outer product "
               "(outerprod_csrsinglecol_by_dvec, R/matmul.R:659-752), which is not on the accelerated path.")
# (taken on the device under options["mxgpu.outer_route"]: outerprod_csrsinglecol_by_dvec below)


def _gemv_csr_svec(x, y):
    """The sparse branch of gemv_csr_vec, R/matmul.R:595-646: x and y sorted (copies, unless MatrixExtra.inplace_sort
    lets a dgRMatrix / the vector be sorted where they are), then matmul_csr_svec_* by the vector's class."""
    if x.Dim[1] != len(y):
        stop("Matrix-vector dimensions do not match.")
    nthreads = options.get("MatrixExtra.nthreads", 1)
    check_valid_matrix(x)
    inplace_sort = bool(options.get("MatrixExtra.inplace_sort", False))
    if inplace_sort and not isinstance(x, dgRMatrix):                 # deepcopy_before_sort, R/utils.R:164-191
        x = x.copy()
    x = as_csr_matrix(x)
    x = sort_sparse_indices(x, copy=not inplace_sort)
    y = sort_sparse_indices(y, copy=not inplace_sort)
    if isinstance(y, dsparseVector):
        res = exports.matmul_csr_svec_numeric(x.p, x.j, x.x, y.i, y.x, nthreads)
    elif isinstance(y, isparseVector):
        res = exports.matmul_csr_svec_integer(x.p, x.j, x.x, y.i, y.x, nthreads)
    elif isinstance(y, lsparseVector):
        res = exports.matmul_csr_svec_logical(x.p, x.j, x.x, y.i, y.x, nthreads)
    elif isinstance(y, nsparseVector):
        res = exports.matmul_csr_svec_binary(x.p, x.j, x.x, y.i, nthreads)
    else:
        return gemv_csr_vec(x, y.toarray())                           # as.numeric(y), :641-644
    return DenseMatrix(res.reshape(-1, 1), [dimnames_of(x)[0], None])


# ---- outer products and float32 vector forms (outer.hip) ------------------------------------------
def _outer_route():
    """The routes below are taken only under options["mxgpu.outer_route"]; without it every refusal stays."""
    return bool(options.get("mxgpu.outer_route", False))


def _names(v):
    """names(v) of a vector operand: its `names` attribute when it carries one"""
    return getattr(v, "names", None)


def _outer_csr(res, Dim, Dimnames):
    return dgRMatrix(res["indptr"], res["indices"], res["values"], Dim, Dimnames)


def _outer_csc(res, Dim, Dimnames):
    return dgCMatrix(res["indptr"], res["indices"], res["values"], Dim, Dimnames)


def outerprod_csrsinglecol_by_dvec(x, y):
    """A one-column RsparseMatrix %*% vector or sparseVector — R/matmul.R:659-744: a dgCMatrix of nrow(x) x length(y)
    for a sparse y, a dgRMatrix for a dense one."""
    if x.Dim[1] != 1:
        stop("Internal error. Please open an issue in GitHub describing what you were doing.")
    x = as_csr_matrix(x)                                              # :663-668: anything but a plain dgRMatrix
    check_valid_matrix(x)
    rn = dimnames_of(x)[0]
    if isinstance(y, sparseVector):
        inplace_sort = bool(options.get("MatrixExtra.inplace_sort", False))
        if type(y) not in (dsparseVector, isparseVector, lsparseVector, nsparseVector):
            return outerprod_csrsinglecol_by_dvec(x, as_sparse_vector(y))        # as(y, "dsparseVector"), :710-713
        y = sort_sparse_indices(y, copy=not inplace_sort)
        if isinstance(y, dsparseVector):
            res = exports.matmul_spcolvec_by_scolvecascsr_numeric(x.p, x.j, x.x, y.i, y.x, y.length)
        elif isinstance(y, isparseVector):
            res = exports.matmul_spcolvec_by_scolvecascsr_integer(x.p, x.j, x.x, y.i, y.x, y.length)
        elif isinstance(y, lsparseVector):
            res = exports.matmul_spcolvec_by_scolvecascsr_logical(x.p, x.j, x.x, y.i, y.x, y.length)
        else:
            res = exports.matmul_spcolvec_by_scolvecascsr_binary(x.p, x.j, x.x, y.i, y.length)
        return _outer_csc(res, (x.Dim[0], y.length), [rn, None])     # :714-720
    names = _names(y)
    yv = np.asarray(y)
    if yv.ndim != 1:
        stop("Matrix-vector dimensions do not match.")
    if yv.dtype != np.float64:                                        # mode(y) <- "double", :723-724
        yv = np.where(yv == NA_INTEGER, NA_REAL, yv.astype(np.float64)) if yv.dtype == np.int32 \
            else yv.astype(np.float64)
    res = exports.matmul_colvec_by_scolvecascsr(yv, x.p, x.j, x.x)
    return _outer_csr(res, (x.Dim[0], yv.size), [rn, names])         # :732-741


def matmul_csr_vec(x, y):
    """RsparseMatrix %*% numeric / logical / integer / sparseVector — R/matmul.R:746-767."""
    if x.Dim[1] == 1:
        return outerprod_csrsinglecol_by_dvec(x, y)
    return gemv_csr_vec(x, y)


def _gemm_csr_f32_vec(x, y):
    """The vector branch of gemm_csr_f32, R/matmul.R:478-505."""
    if x.Dim[1] != 1:
        return gemv_csr_vec(x, y)
    x = as_csr_matrix(x)
    check_valid_matrix(x)
    res = exports.matmul_colvec_by_scolvecascsr_f32(y.Data, x.p, x.j, x.x)
    return _outer_csr(res, (x.Dim[0], y.Data.size), [dimnames_of(x)[0], _names(y)])


def _f32_outer_csc(x, res, ncol, y):
    """R/matmul.R:232-241 / :339-348: a dgCMatrix of length(x) x ncol that takes y's column names, or names(x) when
    x carries some (the reference sets them as the column names)."""
    names = _names(x)
    return _outer_csc(res, (x.Data.size, ncol), [None, names if names is not None else dimnames_of(y)[1]])


def _rowvec_by_sparse(x, p, idx, values):
    if values is not None:
        return float32(exports.matmul_rowvec_by_csc(x.Data, p, idx, values))
    return float32(exports.matmul_rowvec_by_cscbin(x.Data, p, idx))


def _gemm_f32vec_csc(x, y):
    """The vector branch of gemm_f32_csc, R/matmul.R:209-262: to match base R, x is [n, 1] when y has one row and
    [1, n] otherwise."""
    check_valid_matrix(y)
    if y.Dim[0] == 1:
        res = exports.matmul_colvec_by_scolvecascsr_f32(x.Data, y.p, y.i, y.x)
        return _f32_outer_csc(x, res, y.Dim[1], y)
    if y.Dim[0] != x.Data.size:
        stop("(row) vector-Matrix multiplication dimensions do not match.")
    return _rowvec_by_sparse(x, y.p, y.i, y.x)


def _tcrossprod_f32vec_csr(x, y):
    """The vector branch of tcrossprod_f32_csr, R/matmul.R:316-367: x is [n, 1] when y has one column, else [1, n]
    (no dimension check in the reference; the export refuses an index outside the vector)."""
    if y.x is not None and not isinstance(y, dgRMatrix):
        y = as_csr_matrix(y)
    check_valid_matrix(y)
    if y.Dim[1] == 1:
        y = as_csr_matrix(y)
        check_valid_matrix(y)
        res = exports.matmul_colvec_by_scolvecascsr_f32(x.Data, y.p, y.j, y.x)
        return _f32_outer_csc(x, res, y.Dim[0], y)
    return _rowvec_by_sparse(x, y.p, y.j, y.x)


def crossprod_f32_csc(x, y):
    """crossprod(float32 vector, CsparseMatrix) — R/matmul.R:395-430."""
    if x.Data.size != y.Dim[0]:
        stop("(column) vector-Matrix crossprod dimensions do not match.")
    check_valid_matrix(y)
    return _rowvec_by_sparse(x, y.p, y.i, y.x)


# ---- transposed products on the column order (include/mxgpu_tprod.h) -------------------------------
# The reference leaves these signatures to Matrix; here they run on X's CSR arrays through the cached column order.
# A dgCMatrix is read as the CSR of its transpose, so `CsparseMatrix %*% dense` is the transposed product on its arrays.
def _dense_array(o):
    """The dense operand of a transposed product as an array (a base-R vector or matrix), or None for anything else: a
    float32, a sparse matrix or vector."""
    from .structured import StructuredMatrix
    if isinstance(o, (float32, RsparseMatrix, dgCMatrix, sparseVector, StructuredMatrix)) or hasattr(o, "Dim"):
        return None
    a = np.asarray(o)
    return a if a.ndim in (1, 2) and a.dtype.kind in "fiub" else None


def _as_double(y):
    """mode(y) <- "double": an integer or logical operand becomes double, NA becoming NA_real_"""
    y = np.asarray(y)
    if y.dtype == np.float64:
        return y
    if y.dtype == np.int32:
        return np.where(y == NA_INTEGER, NA_REAL, y.astype(np.float64))
    return y.astype(np.float64)


def _tmatvec(p, idx, x, ncols, v):
    """t(S) %*% v for the CSR arrays (p, idx, x) of S with `ncols` columns"""
    v = _as_double(v)
    if v.ndim != 1 or v.size != p.size - 1:
        stop("Matrix-vector dimensions do not match.")
    return exports.csr_tmatvec(p, idx, x, ncols, v)


def crossprod_csr_dense(x, y):
    """crossprod(RsparseMatrix, matrix): t(X) %*% Y, a K x n matrix."""
    check_dimensions_match(x, y, crossprod=True)
    y_names = dimnames_of(y)
    x = as_csr_matrix(x)
    check_valid_matrix(x)
    yd = _as_double(y)
    res = exports.csr_tmatmul_dense(x.p, x.j, x.x, x.Dim[1], np.ascontiguousarray(yd), True)
    return set_dimnames(res, x, DenseMatrix(yd, y_names), crossprod=True)


def crossprod_csr_vec(x, y):
    """crossprod(RsparseMatrix, numeric / integer / logical vector): t(X) %*% v, a K x 1 matrix."""
    x = as_csr_matrix(x)
    check_valid_matrix(x)
    res = _tmatvec(x.p, x.j, x.x, x.Dim[1], y)
    return DenseMatrix(res.reshape(-1, 1), [dimnames_of(x)[1], None])


def gemv_vec_csr(x, y):
    """vector %*% RsparseMatrix: the vector as a row, a 1 x K matrix."""
    y = as_csr_matrix(y)
    check_valid_matrix(y)
    res = _tmatvec(y.p, y.j, y.x, y.Dim[1], x)
    return DenseMatrix(res.reshape(1, -1), [None, dimnames_of(y)[1]])


def gemm_dense_csr(x, y):
    """matrix %*% RsparseMatrix = t(t(Y) %*% t(X)): X's column-major buffer is the row-major t(X), so nothing is
    transposed on the host, and the row-major result is the column-major product."""
    check_dimensions_match(x, y, matmult=True)
    x_names = dimnames_of(x)
    xd = np.asfortranarray(_as_double(x))
    y = as_csr_matrix(y)
    check_valid_matrix(y)
    res = exports.csr_tmatmul_dense(y.p, y.j, y.x, y.Dim[1], xd.T, False)
    return set_dimnames(res.T, DenseMatrix(xd, x_names), y, matmult=True)


def gemm_csc_dense(x, y):
    """CsparseMatrix %*% matrix: the CSC arrays are the CSR of t(X), so this is the transposed product on them."""
    check_dimensions_match(x, y, matmult=True)
    y_names = dimnames_of(y)
    x = as_csc_matrix(x)
    check_valid_matrix(x)
    yd = _as_double(y)
    res = exports.csr_tmatmul_dense(x.p, x.i, x.x, x.Dim[0], np.ascontiguousarray(yd), True)
    return set_dimnames(res, x, DenseMatrix(yd, y_names), matmult=True)


def gemv_csc_vec(x, y):
    """CsparseMatrix %*% numeric / integer / logical vector, an nrow x 1 matrix."""
    x = as_csc_matrix(x)
    check_valid_matrix(x)
    res = _tmatvec(x.p, x.i, x.x, x.Dim[0], y)
    return DenseMatrix(res.reshape(-1, 1), [dimnames_of(x)[0], None])


def tcrossprod_dense_csc(x, y):
    """tcrossprod(matrix, CsparseMatrix): Y %*% t(X) = t(X %*% t(Y)), with X read through its CSC arrays and Y's
    column-major buffer as the row-major t(Y)."""
    check_dimensions_match(x, y, tcrossprod=True)
    x_names = dimnames_of(x)
    xd = np.asfortranarray(_as_double(x))
    y = as_csc_matrix(y)
    check_valid_matrix(y)
    res = exports.csr_tmatmul_dense(y.p, y.i, y.x, y.Dim[0], xd.T, False)
    return set_dimnames(res.T, DenseMatrix(xd, x_names), y, tcrossprod=True)


# ---- sparse x sparse products (include/mxgpu_spgemm.h) ----------------------------------------------
# The reference leaves these signatures to Matrix as well.  They are taken only under options["mxgpu.spgemm_route"];
# without it every call below stops as it always did.
def _spgemm_route():
    return bool(options.get("mxgpu.spgemm_route", False))


def _is_sparse_matrix(o):
    return isinstance(o, (RsparseMatrix, dgCMatrix))


def spgemm_flags(signature, layout_x, layout_y):
    """(trans_a, trans_b, swap) of the one export call behind `signature` ("matmult", "crossprod", "tcrossprod") for
    operands held as "R" (CSR arrays) or "C" (CSC arrays, which are the CSR of the transpose: a flag, not a
    conversion).  The flags are relative to the arrays as they are.  Two CSC operands give a dgCMatrix: its arrays are
    the CSR of the transposed product t(op(y)) t(op(x)), so the operands swap and both flags flip; C1 %*% C2 is then
    the plain product of C2's arrays by C1's, with no transpose at all."""
    ta = (signature == "crossprod") != (layout_x == "C")
    tb = (signature == "tcrossprod") != (layout_y == "C")
    if layout_x == "C" and layout_y == "C":
        return (not tb, not ta, True)
    return (ta, tb, False)


def _raw_csr(o):
    """(indptr, indices, values, dims of the CSR that the arrays spell, layout)"""
    if isinstance(o, dgCMatrix):
        return o.p, o.i, o.x, (o.Dim[1], o.Dim[0]), "C"
    return o.p, o.j, o.x, o.Dim, "R"


def _with_sorted_rows(p, idx, x, dims):
    """the right-hand arrays with every row sorted: as they are when they are sorted, else sorted copies through
    sort_sparse_indices"""
    if exports.check_indices_are_sorted(p, idx):
        return p, idx, x, dims
    cls = ngRMatrix if x is None else lgRMatrix if x.dtype == np.int32 else dgRMatrix
    S = sort_sparse_indices(cls(p, idx, x, dims), copy=True)
    return S.p, S.j, S.x, dims


def spgemm_sparse(x, y, signature):
    """op(x) %*% op(y) for two sparse matrices (RsparseMatrix of any kind, dgCMatrix) on the device: a dgRMatrix, or a
    dgCMatrix when both operands are dgCMatrix.  l and n operands count as numeric (NA -> NA_real_, a pattern entry is
    1), which is Matrix's rule under %*%; nothing is dropped from the result."""
    check_dimensions_match(x, y, **{signature: True})
    check_valid_matrix(x)
    check_valid_matrix(y)
    *a, lx = _raw_csr(x)
    *b, ly = _raw_csr(y)
    trans_a, trans_b, swap = spgemm_flags(signature, lx, ly)
    if swap:
        a, b = b, a
    b = _with_sorted_rows(*b)
    res = exports.csr_spgemm(*a, trans_a, *b, trans_b)
    Dim = (x.Dim[1] if signature == "crossprod" else x.Dim[0], y.Dim[0] if signature == "tcrossprod" else y.Dim[1])
    names = list(_product_dimnames(x, y, signature == "matmult", signature == "crossprod"))
    return (dgCMatrix if swap else dgRMatrix)(res["indptr"], res["indices"], res["values"], Dim, names)


# ---- the one-triangle Gram product (include/mxgpu_gram.h) -------------------------------------------
# Matrix answers crossprod(x) / tcrossprod(x) of a sparse x with a symmetric matrix.  Under options["mxgpu.spgemm_route"]
# together with options["mxgpu.gram_symmetric"] the one-argument forms do so too; without the second option they return
# the general matrix as before.
def _gram_symmetric():
    return _spgemm_route() and bool(options.get("mxgpu.gram_symmetric", False))


def gram_flags(signature, layout):
    """(trans, uplo, cls) of the one export call behind `signature` ("crossprod" / "tcrossprod") of an operand held as
    "R" (CSR arrays) or "C" (CSC arrays, the CSR of the transpose).  trans and uplo are relative to the arrays as they
    are: t(X) X of a CSC is Y t(Y) of its arrays Y, and the rows of the lower mask, read as columns, are the upper
    triangle.  The result always has uplo "U": a dsRMatrix for "R" (spgemm_sparse's class rule: the arrays' layout
    decides; what Matrix gives for a dgRMatrix cannot be pinned without R), a dsCMatrix for "C"."""
    from .structured import dsCMatrix, dsRMatrix
    trans = (signature == "crossprod") != (layout == "C")
    return (trans, "U", dsRMatrix) if layout == "R" else (trans, "L", dsCMatrix)


def gram_sparse(x, signature):
    """crossprod(x) / tcrossprod(x) of a sparse matrix (RsparseMatrix of any kind, dgCMatrix) as a symmetric matrix that
    stores its upper triangle, computed as that triangle alone.  Unsorted rows are sorted in a copy first, for both
    forms: the right-hand side needs it, and the stored triangle equals the other one of the full product bit for bit
    only on sorted rows."""
    check_valid_matrix(x)
    *a, layout = _raw_csr(x)
    trans, uplo, cls = gram_flags(signature, layout)
    res = exports.csr_gram(*_with_sorted_rows(*a), trans, uplo)
    n = x.Dim[1] if signature == "crossprod" else x.Dim[0]
    names = list(_product_dimnames(x, x, False, signature == "crossprod"))
    return cls(res["indptr"], res["indices"], res["values"], (n, n), names, uplo="U")


class RLogical(np.ndarray):
    """An int32 vector tagged as an R logical ({0,1,NA_LOGICAL}) so `%*%` picks the logical kernel."""
    r_logical = True

    def __new__(cls, data):
        return np.ascontiguousarray(data, dtype=np.int32).view(cls)


# ---- dispatch (setMethod("%*%"/"tcrossprod"/"crossprod", ...)) ----------------------------------------
def _general(o):
    """A symmetric or triangular operand as the general class of its layout, as R/matmul.R reaches it through
    as.csr.matrix / as.csc.matrix; anything else as it is."""
    from .structured import StructuredMatrix
    if not isinstance(o, StructuredMatrix):
        return o
    return as_csr_matrix(o) if o.layout == "R" else as_csc_matrix(o)


def matmul(x, y):
    """`%*%` for the signatures the hot path registers (R/matmul.R:200,281,469,512,755-767), and vector | matrix %*%
    RsparseMatrix and CsparseMatrix %*% vector | matrix on the transposed product."""
    x, y = _general(x), _general(y)
    if _spgemm_route() and _is_sparse_matrix(x) and _is_sparse_matrix(y):
        return spgemm_sparse(x, y, "matmult")
    if isinstance(x, RsparseMatrix):
        outer = _outer_route()
        if isinstance(y, float32):
            if y.is_vector:
                return _gemm_csr_f32_vec(x, y) if outer else gemv_csr_vec(x, y)
            return gemm_csr_f32(x, y)
        if isinstance(y, sparseVector):               # R/matmul.R:755-767: one column -> the outer product
            if x.Dim[1] == 1:
                if outer:
                    return outerprod_csrsinglecol_by_dvec(x, y)
                stop(_SVEC_OUTER)
            return gemv_csr_vec(x, y)
        y_arr = np.asarray(y)
        if y_arr.ndim == 1:
            return matmul_csr_vec(x, y) if outer else gemv_csr_vec(x, y)
        return gemm_csr_dense(x, y)
    if isinstance(y, dgCMatrix):
        if isinstance(x, float32) and x.is_vector and _outer_route():
            return _gemm_f32vec_csc(x, y)
        return gemm_f32_csc(x, y) if isinstance(x, float32) else gemm_dense_csc(x, y)
    if isinstance(y, RsparseMatrix) and _dense_array(x) is not None:       # vector | matrix %*% RsparseMatrix
        return gemv_vec_csr(x, y) if _dense_array(x).ndim == 1 else gemm_dense_csr(x, y)
    if isinstance(x, dgCMatrix) and _dense_array(y) is not None:           # CsparseMatrix %*% vector | matrix
        return gemv_csc_vec(x, y) if _dense_array(y).ndim == 1 else gemm_csc_dense(x, y)
    stop("Unsupported operand types for %*% in the MI355X hot path.")


def _one_argument(x, what):
    """crossprod(x) / tcrossprod(x) under options["mxgpu.spgemm_route"]: x as its general class, expanded once and
    taken for both sides; the usual stop without the option, and for anything but a sparse matrix"""
    x = _general(x) if _spgemm_route() else x
    if not (_spgemm_route() and _is_sparse_matrix(x)):
        stop("Unsupported operand types for %s in the MI355X hot path." % what)
    return x


def tcrossprod(x, y=None):
    """tcrossprod for (Rsparse, matrix|float32) and (matrix|float32, Rsparse) — R/matmul.R:307,385,461,538; and
    (matrix, CsparseMatrix) on the transposed product.  Two sparse matrices, and tcrossprod(x) of one, under
    options["mxgpu.spgemm_route"]; with options["mxgpu.gram_symmetric"] as well, tcrossprod(x) is a symmetric matrix."""
    if y is None:
        x = y = _one_argument(x, "tcrossprod")
        if _gram_symmetric():
            return gram_sparse(x, "tcrossprod")
    x, y = _general(x), _general(y)
    if _spgemm_route() and _is_sparse_matrix(x) and _is_sparse_matrix(y):
        return spgemm_sparse(x, y, "tcrossprod")
    if isinstance(x, RsparseMatrix):
        return tcrossprod_csr_f32(x, y) if isinstance(y, float32) else tcrossprod_csr_dense(x, y)
    if isinstance(y, RsparseMatrix):
        if isinstance(x, float32) and x.is_vector and _outer_route():
            return _tcrossprod_f32vec_csr(x, y)
        return tcrossprod_f32_csr(x, y) if isinstance(x, float32) else tcrossprod_dense_csr(x, y)
    if isinstance(y, dgCMatrix) and _dense_array(x) is not None and _dense_array(x).ndim == 2:
        return tcrossprod_dense_csc(x, y)
    stop("Unsupported operand types for tcrossprod in the MI355X hot path.")


def crossprod(x, y=None):
    """crossprod(matrix, CsparseMatrix) — R/matmul.R:393; (float32 vector, CsparseMatrix) — :434, under
    options["mxgpu.outer_route"]; (RsparseMatrix, vector | matrix) on the transposed product.  Two sparse matrices, and
    crossprod(x) of one, under options["mxgpu.spgemm_route"]: the general matrix, or with options["mxgpu.gram_symmetric"]
    as well the symmetric one Matrix gives (gram_sparse)."""
    if y is None:
        x = y = _one_argument(x, "crossprod")
        if _gram_symmetric():
            return gram_sparse(x, "crossprod")
    x, y = _general(x), _general(y)
    if _spgemm_route() and _is_sparse_matrix(x) and _is_sparse_matrix(y):
        return spgemm_sparse(x, y, "crossprod")
    if isinstance(y, dgCMatrix) and isinstance(x, float32) and x.is_vector and _outer_route():
        return crossprod_f32_csc(x, y)
    if isinstance(y, dgCMatrix) and not isinstance(x, float32):
        return crossprod_dense_csc(x, y)
    if isinstance(x, RsparseMatrix) and _dense_array(y) is not None:       # crossprod(RsparseMatrix, vector | matrix)
        return crossprod_csr_vec(x, y) if _dense_array(y).ndim == 1 else crossprod_csr_dense(x, y)
    stop("Unsupported operand types for crossprod in the MI355X hot path.")
