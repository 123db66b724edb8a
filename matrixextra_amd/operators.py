"""Host-side mirror of the CSR (+) CSR part of R/operators.R
(multiply_csr_by_csr :43-79, add_csr_matrices_internal :713-776 and their registrations), of CSR (.) COO
(multiply_csr_by_coo :81-110), of `CSC * matrix` (multiply_csc_by_dense_internal :568-670) and of `CSR op vector` /
`COO op vector` (multiply_csr_by_dvec_elemwise_internal :950-1153), of `CSR * sparseVector`
(multiply_csr_by_svec_elemwise_internal :1564-1622), of `matrix * sparseVector`
(multiply_elemwise_dense_by_svec_internal :1641-1682) and of `COO * matrix` (multiply_coo_by_dense_internal :400-483)."""
from __future__ import annotations

import warnings

import numpy as np

from . import exports
from .matrices import (NA_INTEGER, RsparseMatrix, TsparseMatrix, as_coo_matrix, as_csc_matrix, as_csr_matrix, as_sparse_vector,
                       check_valid_matrix, dgCMatrix, dgRMatrix, dgTMatrix, dsparseVector, float32, lgRMatrix, lgTMatrix,
                       ngRMatrix, nsparseVector, options, sort_sparse_indices, sparseVector,
                       stop)


def _is_same_ngRMatrix(e1, e2):
    """is_same_ngRMatrix (src/misc.cpp:108-116): pointer identity of p and j."""
    return (e1.p.ctypes.data == e2.p.ctypes.data and e1.j.ctypes.data == e2.j.ctypes.data
            and e1.p.size == e2.p.size and e1.j.size == e2.j.size)


def _deepcopy_before_sort(e):
    return e.copy()


def _prepare(e, logical):
    """check_valid_matrix; [deepcopy]; as.csr.matrix; sort_sparse_indices — R/operators.R:54-64, :744-754."""
    if not isinstance(e, RsparseMatrix):
        e = as_csr_matrix(e, logical=logical)
    inplace_sort = bool(options.get("MatrixExtra.inplace_sort", False))
    check_valid_matrix(e)
    if inplace_sort:
        e = _deepcopy_before_sort(e)
    e = as_csr_matrix(e, logical=logical)
    return sort_sparse_indices(e, copy=not inplace_sort)


def _assemble(cls, e1, res):
    out = cls.__new__(cls)
    out.Dim = e1.Dim
    out.Dimnames = list(e1.Dimnames)
    out.p = res["indptr"]
    out.j = res["indices"]
    out.x = res["values"]
    return out


def multiply_csr_by_csr(e1, e2, logical=False):
    """R/operators.R:43-79."""
    if e1.Dim[0] != e2.Dim[0] or e1.Dim[1] != e2.Dim[1]:
        stop("Matrices must have the same dimensions in order to multiply them.")
    if isinstance(e1, ngRMatrix) and isinstance(e2, ngRMatrix) and _is_same_ngRMatrix(e1, e2):
        return e1
    e1 = _prepare(e1, logical)
    e2 = _prepare(e2, logical)
    if not logical:
        res = exports.multiply_csr_elemwise(e1.p, e2.p, e1.j, e2.j, e1.x, e2.x)
        return _assemble(dgRMatrix, e1, res)
    res = exports.logicaland_csr_elemwise(e1.p, e2.p, e1.j, e2.j, e1.x, e2.x)
    return _assemble(lgRMatrix, e1, res)


def multiply_csr_by_coo(e1, e2, logical=False):
    """R/operators.R:81-110: CSR `e1` times (or AND) COO `e2`, one output triplet per kept COO entry, in e2's
    order; Dim is the elementwise max of the two, no Dimnames."""
    if e1.Dim[0] != e2.Dim[0] or e1.Dim[1] != e2.Dim[1]:
        warnings.warn("Matrices to multiply have different dimensions.")
    e1 = _prepare(e1, logical)
    e2 = as_coo_matrix(e2, logical=logical)
    check_valid_matrix(e2)
    fn = exports.logicaland_csr_by_coo_elemwise if logical else exports.multiply_csr_by_coo_elemwise
    res = fn(e1.p, e1.j, e1.x, e2.i, e2.j, e2.x, e1.Dim[0], e1.Dim[1])
    cls = lgTMatrix if logical else dgTMatrix
    return cls(res["row"], res["col"], res["val"], (max(e1.Dim[0], e2.Dim[0]), max(e1.Dim[1], e2.Dim[1])))


def add_csr_matrices_internal(e1, e2, is_substraction=False, is_ampersand=False, is_xor=False):
    """R/operators.R:713-776 (`is_ampersand` is the reference's name for the `|` path)."""
    if e1.Dim[0] != e2.Dim[0] or e1.Dim[1] != e2.Dim[1]:
        stop("Matrices must have the same dimensions in order to add/substract them.")
    logical = is_ampersand or is_xor
    if isinstance(e1, ngRMatrix) and isinstance(e2, ngRMatrix) and _is_same_ngRMatrix(e1, e2):
        if not is_substraction and not is_xor:
            return e1
        if is_xor:
            return lgRMatrix(np.zeros(e1.Dim[0] + 1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                             np.zeros(0, dtype=np.int32), e1.Dim, e1.Dimnames)
        # R/operators.R:731-738 (sic: the reference fills 2.0 on this branch)
        return dgRMatrix(e1.p, e1.j, np.full(e1.j.size, 2.0), e1.Dim, e1.Dimnames)
    e1 = _prepare(e1, logical)
    e2 = _prepare(e2, logical)
    if not logical:
        res = exports.add_csr_elemwise(e1.p, e2.p, e1.j, e2.j, e1.x, e2.x, is_substraction)
        return _assemble(dgRMatrix, e1, res)
    res = exports.logicalor_csr_elemwise(e1.p, e2.p, e1.j, e2.j, e1.x, e2.x, bool(is_xor))
    return _assemble(lgRMatrix, e1, res)


def add_csr_matrices(e1, e2, is_substraction=False):
    """R/operators.R:778-780."""
    return add_csr_matrices_internal(e1, e2, is_substraction, False, False)


def logicalor_csr_matrices(e1, e2):
    """R/operators.R:782-784."""
    return add_csr_matrices_internal(e1, e2, False, True, False)


def xor_csr_matrices(e1, e2):
    """R/operators.R:786-788."""
    return add_csr_matrices_internal(e1, e2, False, False, True)


_NOT_ACCELERATED = ("This combination takes the reference's NA / dense route "
                    "(multiply_csr_by_dvec_with_NAs or a CsparseMatrix fallback, R/operators.R:%s), "
                    "which is not on the accelerated path.")


_CSC_AND = "CsparseMatrix & matrix would give an lgCMatrix, which this package does not provide."
_CSC_VECTOR = ("CsparseMatrix * vector is Matrix's own method (MatrixExtra registers `*` only for a CsparseMatrix "
               "and a matrix or float32, R/operators.R:673-689), which is not on the accelerated path.")


def _recycle_float32_vector(e1, e2):
    """recycle_float32_vector (R/operators.R:219-235): the vector becomes a one-column matrix; when e1 has more
    columns, the vector is repeated ncol(e1) times down that one column (sic), so only a one-column e1 passes the
    dimension check that follows."""
    data = e2.Data.reshape(-1, 1)
    if data.shape[1] < e1.Dim[1]:
        data = np.tile(data.reshape(-1), e1.Dim[1] // data.shape[1]).reshape(-1, 1)
    return float32(data)


def _csc_dense_operand(e2):
    """(dense array, kind) of the right operand, by R's typeof(e2) (R/operators.R:599-610, 634-645): float64 numeric,
    int32 integer, bool or RLogical logical, float32 its @Data; any other type goes through as.double (`mode(e2) <-
    "double"`)."""
    if isinstance(e2, float32):
        return e2.Data, "float32"
    a = np.asarray(e2)
    if a.ndim != 2:
        stop(_CSC_VECTOR)
    if getattr(e2, "r_logical", False) or a.dtype == np.bool_:
        return a, "logical"
    if a.dtype == np.float64:
        return a, "numeric"
    if a.dtype == np.int32:
        return a, "integer"
    return a.astype(np.float64), "numeric"


_CSC_IGNORE = {"numeric": "multiply_csc_by_dense_ignore_NAs_numeric", "integer": "multiply_csc_by_dense_ignore_NAs_integer",
               "logical": "multiply_csc_by_dense_ignore_NAs_logical", "float32": "multiply_csc_by_dense_ignore_NAs_float32"}
_CSC_KEEP = {"numeric": "multiply_csc_by_dense_keep_NAs_numeric", "integer": "multiply_csc_by_dense_keep_NAs_integer",
             "logical": "multiply_csc_by_dense_keep_NAs_logical", "float32": "multiply_csc_by_dense_keep_NAs_float32"}


def multiply_csc_by_dense_internal(e1, e2, logical=False):
    """R/operators.R:568-661 for a dgCMatrix `e1` and a dense `e2` (ndarray, DenseMatrix or float32): `e1 * e2`, a
    dgCMatrix with e1's Dim and Dimnames.  Under MatrixExtra.ignore_na the values-only route keeps e1's `p` object and
    a copy of `i`; otherwise the columns are sorted (a copy, or e1's own arrays under MatrixExtra.inplace_sort) and
    every NA cell of e2 outside e1's pattern becomes an NA_real_ entry.  `&` would give an lgCMatrix and raises."""
    if logical:
        stop(_CSC_AND)
    ignore_NAs = bool(options.get("MatrixExtra.ignore_na", False))                # :570
    if isinstance(e2, float32) and e2.is_vector:                                   # :572-589
        n2, nrow = e2.Data.size, e1.Dim[0]
        if n2 == 0:
            return np.zeros(0, dtype=np.float64)
        if n2 > nrow * e1.Dim[1]:
            stop("Vector to multiply with has more entries than matrix dimensions.")
        if n2 > nrow or (n2 < nrow and n2 % nrow) or (n2 != nrow and not ignore_NAs and bool(np.isnan(e2.Data).any())):
            stop(_NOT_ACCELERATED % "585")                                         # e1 * float::dbl(e2): Matrix's
        e2 = _recycle_float32_vector(e1, e2)
    D, kind = _csc_dense_operand(e2)
    if e1.Dim[0] != D.shape[0] or e1.Dim[1] != D.shape[1]:                         # :591-592
        stop("Matrices must have the same dimensions in order to multiply them.")
    check_valid_matrix(e1)
    e1 = as_csc_matrix(e1)
    out = dgCMatrix.__new__(dgCMatrix)
    out.Dim, out.Dimnames = e1.Dim, list(e1.Dimnames)
    if ignore_NAs:                                                                 # :595-622
        out.x = getattr(exports, _CSC_IGNORE[kind])(e1.p, e1.i, e1.x, D)
        out.p, out.i = e1.p, e1.i.copy()
        return out
    if not options.get("MatrixExtra.inplace_sort", False):                         # :626-630
        e1 = dgCMatrix(e1.p, e1.i.copy(), e1.x.copy(), e1.Dim, e1.Dimnames)
    exports.sort_sparse_indices_inplace(e1.p, e1.i, e1.x)                          # per column
    res = getattr(exports, _CSC_KEEP[kind])(e1.p, e1.i, e1.x, D)                   # :632-659
    out.p, out.i, out.x = res["indptr"], res["indices"], res["values"]
    return out


def multiply_csc_by_dense(e1, e2):
    """R/operators.R:663-665 (also `matrix * CsparseMatrix` and `float32 * CsparseMatrix`, :681-689)."""
    return multiply_csc_by_dense_internal(e1, e2, False)


def logicaland_csc_by_dense(e1, e2):
    """R/operators.R:667-669, registered for `&` at :693-709: the result would be an lgCMatrix."""
    return multiply_csc_by_dense_internal(e1, e2, True)


def _as_logical(v):
    """as.logical() for a numeric / bool vector -> R logical (int32 with NA_LOGICAL)."""
    v = np.asarray(v)
    if v.dtype == np.int32:
        return v
    if v.dtype.kind == "f":
        return np.where(np.isnan(v), np.int32(-2147483648), (v != 0).astype(np.int32)).astype(np.int32)
    return (v != 0).astype(np.int32)


def _csr_by_dvec_keep_na_route(e1, e2, X_is_LHS, op):
    """The take_route_NAs branch of R/operators.R:996-1129, taken under options["mxgpu.dvec_na_route"]: `e2` (float64)
    holds an NA / NaN, a zero under / %% %/% ^, an Inf under * or a negative exponent under ^, and the cells that R
    makes NA / NaN / 1 / Inf outside e1's pattern are added (multiply_csr_by_dvec_with_NAs).  The result is a
    dgRMatrix with e1's Dim and Dimnames; e1 is sorted in a copy unless MatrixExtra.inplace_sort is set.  What the
    reference hands to a CsparseMatrix here (a vector that is all NA, a vector of length one) raises."""
    if bool(np.isnan(e2).all()):                                              # :998-1006
        stop(_NOT_ACCELERATED % "998-1006")
    if isinstance(e1, TsparseMatrix):                                         # :1008-1011
        e1 = as_csr_matrix(e1, logical=False)
    inplace_sort = bool(options.get("MatrixExtra.inplace_sort", False))
    if inplace_sort:                                                          # :1013-1014
        e1 = _deepcopy_unless_numeric(e1)
    e1 = as_csr_matrix(e1, logical=False)                                     # :1022-1030
    if e2.size == 1:                                                          # always one of the CsparseMatrix fallbacks
        if op == "*":
            stop(_NOT_ACCELERATED % "1052-1056")
        if op in ("/", "%%", "%/%"):
            if X_is_LHS:
                warnings.warn("Warning: division by zero.")
            stop(_NOT_ACCELERATED % "1063-1069")
        stop(_NOT_ACCELERATED % "1085-1089")
    e1 = sort_sparse_indices(e1, copy=not inplace_sort)                       # :1112-1114
    if e1.Dim[0] % e2.size != 0:                                              # :1116-1117
        warnings.warn("Number of elements in vector is not a multiple of matrix dimension.")
    res = exports.multiply_csr_by_dvec_with_NAs(e1.p, e1.j, e1.x, e2, e1.Dim[1], op == "*", op == "^", op == "/",
                                                op == "%%", op == "%/%", X_is_LHS)   # :1119-1129
    return _assemble(type(e1), e1, res)


def multiply_csr_by_dvec_elemwise_internal(e1, e2, logical=False, X_is_LHS=True, op="*"):
    """R/operators.R:950-1153 for RsparseMatrix or TsparseMatrix `e1`: `e1 op e2` (or `e2 op e1` when X_is_LHS is false) with a dense
    vector (or a same-shape dense matrix read as a vector), R's recycling, values-only result.  The routes the
    reference sends through multiply_csr_by_dvec_with_NAs or through a CsparseMatrix (vector with NA, division by
    zero, multiplication by Inf, `v op X` for ^ / %% %/% while NAs are kept) raise, unless
    options["mxgpu.dvec_na_route"] is set: then the first of them runs on the device (_csr_by_dvec_keep_na_route)."""
    e2 = np.asarray(e2)
    if e2.ndim == 2:                                                          # :952-959
        if e1.Dim[0] != e2.shape[0] or e2.shape[1] != e2.shape[1]:            # (sic: the reference compares ncol(e2) with itself)
            stop("Matrix dimensions do not match. Cannot perform the opertion.")
        e2 = e2.reshape(-1, order="F")
    e2 = e2.reshape(-1)
    if e2.size == 0:                                                          # :961-966
        return np.zeros(0, dtype=np.int32 if logical else np.float64)
    if e2.size > e1.Dim[0] * e1.Dim[1]:
        stop("Vector to multiply with has more entries than matrix.")
    keep_NAs = not bool(options.get("MatrixExtra.ignore_na", False))
    if (not X_is_LHS) and keep_NAs and op in ("^", "/", "%%", "%/%"):         # :973-978
        stop(_NOT_ACCELERATED % "973-978")
    check_valid_matrix(e1)
    e2f = e2.astype(np.float64) if e2.dtype != np.int32 else np.where(e2 == np.int32(-2147483648), np.nan, e2.astype(np.float64))
    take_route_NAs = (not logical) and keep_NAs and (
        bool(np.isnan(e2f).any())
        or (op in ("^", "/", "%%", "%/%") and bool((e2f == 0).any()))
        or (op == "*" and bool(np.isinf(e2f).any()))
        or (op == "^" and bool((e2f < 0).any())))                             # :981-988
    if take_route_NAs:
        if not options.get("mxgpu.dvec_na_route", False):
            stop(_NOT_ACCELERATED % "981-1131")
        return _csr_by_dvec_keep_na_route(e1, e2f, X_is_LHS, op)
    e2 = _as_logical(e2) if logical else e2f
    is_coo = isinstance(e1, TsparseMatrix)                                    # :990
    e1 = as_coo_matrix(e1, logical=logical) if is_coo else as_csr_matrix(e1, logical=logical)   # :1020-1029
    out = type(e1).__new__(type(e1))
    if is_coo:
        out.i, out.j = e1.i, e1.j
    else:
        out.p, out.j = e1.p, e1.j
    out.Dim, out.Dimnames = e1.Dim, list(e1.Dimnames)
    if e2.size == 1:                                                          # :1031-1108
        if logical:
            if e2[0] == np.int32(-2147483648):
                out.x = np.where(e1.x == np.int32(-2147483648), np.int32(-2147483648), np.int32(0)).astype(np.int32)
                return out
            if e2[0] == 0:
                if is_coo:
                    return lgTMatrix(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                     np.zeros(0, dtype=np.int32), e1.Dim, e1.Dimnames)
                res = lgRMatrix(np.zeros(e1.Dim[0] + 1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                np.zeros(0, dtype=np.int32), e1.Dim, e1.Dimnames)
                return res
            return e1
        if op in ("/", "%%", "%/%") and e2[0] == 0 and X_is_LHS:
            warnings.warn("Warning: division by zero.")
        if op == "^" and (not X_is_LHS) and (e2[0] == 1 or e2[0] == 0):
            stop(_NOT_ACCELERATED % "1091-1095")
    elif e1.Dim[0] % e2.size != 0:                                            # :1114-1115
        warnings.warn("Number of elements in vector is not a multiple of matrix dimension.")
    if is_coo:                                                                # :1139-1150
        if logical:
            out.x = exports.multiply_coo_by_dense_ignore_NAs_logical(e1.i, e1.j, e1.x, e2, e1.Dim[0], e1.Dim[1])
        else:
            out.x = exports.multiply_coo_by_dense_ignore_NAs_numeric(e1.i, e1.j, e1.x, e2, e1.Dim[0], e1.Dim[1],
                                                                     op == "*", op == "^", op == "/", op == "%%",
                                                                     op == "%/%", X_is_LHS)
    elif logical:
        out.x = exports.logicaland_csr_by_dvec_internal(e1.p, e1.j, e1.x, e2, e1.Dim[1])
    else:
        out.x = exports.multiply_csr_by_dvec_no_NAs_numeric(e1.p, e1.j, e1.x, e2, e1.Dim[1], op == "*", op == "^",
                                                            op == "/", op == "%%", op == "%/%", X_is_LHS)
    return out


def csr_op_vector(e1, e2, op, X_is_LHS=True):
    """`X * v`, `X / v`, `X ^ v`, `X %% v`, `X %/% v`, `X & v` and their mirrored forms (R/operators.R:1155-1215)."""
    if op == "&":
        return multiply_csr_by_dvec_elemwise_internal(e1, e2, logical=True)
    return multiply_csr_by_dvec_elemwise_internal(e1, e2, logical=False, X_is_LHS=X_is_LHS, op=op)


_SVEC_CSC = ("A sparseVector longer than nrow(X), or whose length does not divide nrow(X), goes through as.csc.matrix "
             "and Matrix's own method (R/operators.R:1587-1588), which is not on the accelerated path.")


def _deepcopy_unless_numeric(e):
    """deepcopy_before_sort (R/utils.R:164-191) as the sparse-vector routes use it: an object that is not of the
    numeric kind is about to be converted into one that shares its index array, so it is copied first; a dgRMatrix
    or dsparseVector stays itself and is then sorted in place."""
    return e if isinstance(e, (dgRMatrix, dsparseVector)) else e.copy()


def multiply_csr_by_svec_elemwise_internal(X, v):
    """R/operators.R:1564-1622: `X * v` for an RsparseMatrix and a sparseVector recycled down the rows.  Rows at
    positions that `v` does not store drop out, the stored ones are scaled; unless MatrixExtra.ignore_na is set, the
    NaN / Inf entries of dropped rows stay (as NaN) and a NaN / Inf value of `v` fills its rows.  The result is a
    dgRMatrix with X's Dim and Dimnames."""
    if not len(v):                                                            # :1565-1566
        return np.zeros(0, dtype=np.float64)
    inplace_sort = bool(options.get("MatrixExtra.inplace_sort", False))
    if len(v) == 1 or len(v) == v.i.size:                                     # :1570-1582
        if len(v) == 1:
            dv = v.toarray()
        elif v.x is not None:
            if inplace_sort:
                v = _deepcopy_unless_numeric(v)
            dv = sort_sparse_indices(v, copy=not inplace_sort).x
        else:
            return X
        return csr_op_vector(X, dv, "*")
    if (len(v) < X.Dim[0] and X.Dim[0] % len(v) != 0) or len(v) > X.Dim[0]:  # :1584-1589
        stop(_SVEC_CSC)
    check_valid_matrix(X)
    if inplace_sort:                                                          # :1594-1597
        X = _deepcopy_unless_numeric(X)
        v = _deepcopy_unless_numeric(v)
    X = as_csr_matrix(X)
    X = sort_sparse_indices(X, copy=not inplace_sort)
    v = as_sparse_vector(v, binary=isinstance(v, nsparseVector))              # :1601
    v = sort_sparse_indices(v, copy=not inplace_sort)
    keep_NAs = not bool(options.get("MatrixExtra.ignore_na", False))
    if v.x is not None and keep_NAs:                                          # :1606-1614
        res = exports.multiply_csr_by_svec_keep_NAs(X.p, X.j, X.x, v.i, v.x, X.Dim[1], len(v))
    else:
        res = exports.multiply_csr_by_svec_no_NAs(X.p, X.j, X.x, v.i, v.x, len(v))
    return _assemble(dgRMatrix, X, res)


def multiply_csr_by_svec_elemwise(e1, e2):
    """R/operators.R:1624-1638: `RsparseMatrix * sparseVector` and `sparseVector * RsparseMatrix`."""
    if isinstance(e2, sparseVector):
        return multiply_csr_by_svec_elemwise_internal(e1, e2)
    return multiply_csr_by_svec_elemwise_internal(e2, e1)


_SVEC_DENSE = {"numeric": "multiply_elemwise_dense_by_svec_numeric", "integer": "multiply_elemwise_dense_by_svec_integer",
               "logical": "multiply_elemwise_dense_by_svec_logical", "float32": "multiply_elemwise_dense_by_svec_float32"}


def multiply_elemwise_dense_by_svec_internal(e1, e2):
    """R/operators.R:1641-1682: `e1 * e2` for a dense matrix `e1` (2-d ndarray, DenseMatrix or float32) and a
    sparseVector `e2`.  A vector that covers the cells of e1, or that recycles over them unevenly, gives a dense
    float64 matrix (no dimnames); one whose length divides nrow(e1) gives a dgRMatrix of full rows with e1's Dim and
    Dimnames.  Unless MatrixExtra.ignore_na is set the vector is sorted first (a copy, or in place under
    MatrixExtra.inplace_sort) and the NA / NaN / Inf cells that it does not cover stay as NA / NaN.  An empty operand
    gives R's matrix(): one NA cell."""
    if isinstance(e1, float32):
        data = e1.Data.reshape(-1, 1) if e1.is_vector else e1.Data           # :1661-1662
        nrow1 = data.shape[0]
    else:
        data = np.asarray(e1)
        nrow1 = data.shape[0]
    if not nrow1 or not len(e2):                                              # :1642-1643
        return np.full((1, 1), np.nan)
    keep_NAs = not bool(options.get("MatrixExtra.ignore_na", False))
    inplace_sort = bool(options.get("MatrixExtra.inplace_sort", False))
    if keep_NAs and inplace_sort:                                             # :1647-1648
        e2 = _deepcopy_unless_numeric(e2)
    e2 = as_sparse_vector(e2)
    if keep_NAs:                                                              # :1650-1651
        e2 = sort_sparse_indices(e2, copy=not inplace_sort)
    if isinstance(e1, float32):                                               # :1653-1667, by typeof(e1)
        kind = "float32"
    elif getattr(e1, "r_logical", False) or data.dtype == np.bool_:
        kind = "logical"
    elif data.dtype == np.float64:
        kind = "numeric"
    elif data.dtype == np.int32:
        kind = "integer"
    else:
        data, kind = data.astype(np.float64), "numeric"                       # mode(e1) <- "double"
    res = getattr(exports, _SVEC_DENSE[kind])(data, e2.i, e2.x, len(e2), keep_NAs)
    if "X_dense" in res:                                                      # :1669-1670
        return res["X_dense"]
    out = dgRMatrix.__new__(dgRMatrix)                                        # :1672-1681
    out.Dim = (int(data.shape[0]), int(data.shape[1]))
    out.Dimnames = list(getattr(e1, "Dimnames", None) or [None, None])
    out.p, out.j, out.x = res["indptr"], res["indices"], res["values"]
    return out


def multiply_elemwise_dense_by_svec(e1, e2):
    """R/operators.R:1684-1705: `matrix * sparseVector`, `float32 * sparseVector` and their mirrored forms."""
    if isinstance(e2, sparseVector):
        return multiply_elemwise_dense_by_svec_internal(e1, e2)
    return multiply_elemwise_dense_by_svec_internal(e2, e1)


_INTERNAL_ERROR = "Unexpected error. Please open an issue in GitHub explaining what you were doing."


def multiply_coo_by_dense_internal(e1, e2, logical=False):
    """R/operators.R:400-483: `e1 * e2` / `e1 & e2` for a TsparseMatrix `e1` and a dense matrix `e2`, taken only under
    options["mxgpu.coo_dense_route"].  A double matrix and every `&` go to the vector route
    (multiply_csr_by_dvec_elemwise_internal, :402-403), an integer / logical matrix with an NA while NAs are kept
    goes through as.csc.matrix to the CSC route (:412-415), and an integer or logical matrix without one is gathered
    at the triplets (multiply_coo_by_dense_{integer,logical}): a dgTMatrix with new @i / @j and no Dimnames.  The
    reference tests the wrong operand for float32 (`inherits(e1, "float32")`, :455) and ends in
    throw_internal_error(); so does this."""
    if not isinstance(e2, float32) and not getattr(e2, "r_logical", False) \
            and np.asarray(e2).dtype not in (np.bool_, np.int32, np.float64):
        e2 = np.asarray(e2).astype(np.float64)                                # any other type is R's double
    if logical or (not isinstance(e2, float32) and np.asarray(e2).dtype == np.float64):      # :402-403
        return multiply_csr_by_dvec_elemwise_internal(e1, np.asarray(e2), logical=logical)
    if isinstance(e2, float32) and e2.is_vector and not e2.Data.size:         # :405-410
        return np.zeros(0, dtype=np.float64)
    if isinstance(e2, float32):
        has_na = bool(np.isnan(e2.Data).any())
    else:
        a = np.asarray(e2)
        has_na = bool((a == NA_INTEGER).any()) if a.dtype == np.int32 else False
    if not bool(options.get("MatrixExtra.ignore_na", False)) and has_na:      # :412-415
        return multiply_csc_by_dense_internal(as_csc_matrix(e1), e2, logical)
    if isinstance(e2, float32) and e2.is_vector:                              # :417
        e2 = _recycle_float32_vector(e1, e2)
    shape2 = e2.Data.shape if isinstance(e2, float32) else np.asarray(e2).shape
    if shape2[0] < e1.Dim[0] or shape2[1] < e1.Dim[1]:                        # :418-419
        stop("Cannot multiply matrices elementwise - dimensions do not match.")
    if not isinstance(e1, dgTMatrix):                                         # :421-426
        e1 = as_coo_matrix(e1, logical=False)
    check_valid_matrix(e1)
    if isinstance(e2, float32):                                               # :455-464
        stop(_INTERNAL_ERROR)
    a = np.asarray(e2)
    if getattr(e2, "r_logical", False) or a.dtype == np.bool_:                # :448-454
        res = exports.multiply_coo_by_dense_logical(a, e1.i, e1.j, e1.x)
    elif a.dtype == np.int32:                                                 # :441-447
        res = exports.multiply_coo_by_dense_integer(a, e1.i, e1.j, e1.x)
    else:
        stop(_INTERNAL_ERROR)
    return dgTMatrix(res["row"], res["col"], res["val"],
                     (max(e1.Dim[0], shape2[0]), max(e1.Dim[1], shape2[1])))  # :478-482


def multiply_coo_by_dense(e1, e2):
    """R/operators.R:485-487."""
    return multiply_coo_by_dense_internal(e1, e2, False)


def logicaland_coo_by_dense(e1, e2):
    """R/operators.R:489-491."""
    return multiply_coo_by_dense_internal(e1, e2, True)
