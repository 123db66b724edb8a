"""Mirror of R/rbind.R and R/cbind.R: rbind_csr, rbind2, cbind2 and the left folds rbind / cbind over the stand-in
classes of matrices.py.  Checks, shortcuts, class rules, messages and dimnames are the reference's, cited by line; the
arrays come from the device through exports.py (the batched row concat, the COO concat, cbind of two CSR, a sparse
vector as a column of a CSR, the dense vector compaction).

Defined here rather than by the reference:
  * rbind2 of R / sparseVector / C / T operands that the reference hands to Matrix's cbind2(CSC, CSC) is a two-operand
    row concat with the kind rule and dimnames of the reference's own unreachable rbind2_dgr / lgr / ngr;
  * cbind2(RsparseMatrix, sparseVector) and its mirror image give an RsparseMatrix;
  * dense numeric / integer / logical vectors with an R or C operand: the length must equal the bound dimension or
    be 1, the result is numeric in the sparse operand's format and zeros of the vector are not stored;
  * a sparseVector that a shortcut turns into a matrix becomes one ROW in rbind and one COLUMN in cbind.
"""
from __future__ import annotations

import copy
import functools

import numpy as np

from . import exports
from ._lib import MX_F64, MX_I32, MX_LGL
from .matrices import (NA_LOGICAL, MatrixExtraError, RsparseMatrix, TsparseMatrix, as_coo_matrix, as_csr_matrix,
                       check_valid_matrix, dgCMatrix, dgRMatrix, dgTMatrix, dimnames_of, dsparseVector, isparseVector,
                       lgRMatrix, lgTMatrix, lsparseVector, ngRMatrix, ngTMatrix, nsparseVector, sparseVector, stop,
                       t_shallow)
from .structured import StructuredMatrix, as_general

_INT_MAX = 2147483647                     # .Machine$integer.max
_BINARY = (ngRMatrix, ngTMatrix, nsparseVector)                        # "nsparseMatrix", "nsparseVector"
_LOGICAL = (lgRMatrix, lgTMatrix, lsparseVector)                       # "lsparseMatrix", "lsparseVector"
_CSR_OF_KIND = {"d": dgRMatrix, "l": lgRMatrix, "n": ngRMatrix}
_COO_OF_KIND = {"d": dgTMatrix, "l": lgTMatrix, "n": ngTMatrix}
_OUT = {"d": 0, "l": 1, "n": 2}                                        # out_kind of the device concat
_INTERNAL_ERROR = "Internal error. Please file an issue in GitHub."


# ----------------------------------------------------------------------------------------------- operands
def _is_dense_vector(x):
    if isinstance(x, (list, tuple)):
        return True
    return isinstance(x, np.ndarray) and x.ndim == 1


def _dense_dtype(x):
    """(array, mx dtype) of a dense vector by R's type: logical, integer, else double (as operators.py reads them)"""
    a = np.asarray(x)
    if getattr(x, "r_logical", False) or a.dtype == np.bool_:
        return np.ascontiguousarray(a, dtype=np.int32), MX_LGL
    if a.dtype == np.int32:
        return a, MX_I32
    return np.ascontiguousarray(a, dtype=np.float64), MX_F64


def _dense_as_svec(x, length=None, what="bind"):
    """A dense vector as the dsparseVector the device compaction gives (zeros dropped, NA kept as NA_real_); with
    `length`, the vector must have that length or be of length 1, which is recycled."""
    a, dt = _dense_dtype(x)
    if length is not None and a.size != length:
        if a.size != 1:
            raise MatrixExtraError(f"{what}: the vector has length {a.size}, which is neither 1 nor the matrix's "
                                   f"dimension ({length}).")
        a = np.repeat(a, length)
    res = exports.dense_to_svec(a, dt)
    return dsparseVector(res["ii"], res["xx"], a.size)


def _is_binary(x):
    return isinstance(x, _BINARY) or (isinstance(x, StructuredMatrix) and x.value_dtype is None)


def _is_logical(x):
    return isinstance(x, _LOGICAL) or (isinstance(x, StructuredMatrix) and x.value_dtype == np.int32)


def _expanded(x):
    """a symmetric / triangular operand as the general class of its kind and layout (R/rbind.R:297-306,
    R/cbind.R:83-85: as.csr.matrix with the kind kept); anything else as it is"""
    return as_general(x) if isinstance(x, StructuredMatrix) else x


def _kind2(x, y):
    """:311-317, R/cbind.R:82-99: n + n -> n, {n, l} x {n, l} -> l, else d"""
    if _is_binary(x) and _is_binary(y):
        return "n"
    if (_is_binary(x) or _is_logical(x)) and (_is_binary(y) or _is_logical(y)):
        return "l"
    return "d"


def _csr_kind(x):
    return 0 if isinstance(x, dgRMatrix) else 1 if isinstance(x, lgRMatrix) else 2


def _svec_kind(v):
    return (3 if isinstance(v, dsparseVector) else 4 if isinstance(v, isparseVector)
            else 5 if isinstance(v, lsparseVector) else 6)


def _row_operand(x):
    """the tuple exports.concat_csr_batch takes"""
    if isinstance(x, sparseVector):
        return (_svec_kind(x), None, x.i, x.x, 1)
    return (_csr_kind(x), x.p, x.j, x.x, x.Dim[0])


def _nrow(x):
    return 1 if isinstance(x, sparseVector) else x.Dim[0]


def _ncol(x):
    return x.length if isinstance(x, sparseVector) else x.Dim[1]


def _with_dim(x, Dim):
    out = copy.copy(x)
    out.Dim = (int(Dim[0]), int(Dim[1]))
    out.Dimnames = list(dimnames_of(x))
    if isinstance(x, RsparseMatrix) and out.p.size - 1 < out.Dim[0]:      # keep the slots a valid CSR
        out.p = np.concatenate([x.p, np.full(out.Dim[0] - (x.p.size - 1), x.p[-1], np.int32)])
    if isinstance(x, dgCMatrix) and out.p.size - 1 < out.Dim[1]:
        out.p = np.concatenate([x.p, np.full(out.Dim[1] - (x.p.size - 1), x.p[-1], np.int32)])
    return out


def _svec_as_row(v):
    """as.csr.matrix / as(v, "RsparseMatrix") of a sparse vector in rbind: one row of the vector's kind (an
    isparseVector becomes numeric), through the one-operand device concat"""
    kind = "n" if _is_binary(v) else "l" if _is_logical(v) else "d"
    res = exports.concat_csr_batch([_row_operand(v)], _OUT[kind])
    return _CSR_OF_KIND[kind](res["indptr"], res["indices"], res["values"], (1, v.length))


def _cast_csr_same(x):
    """:29"""
    if isinstance(x, sparseVector):
        return _svec_as_row(x)
    return as_csr_matrix(x, binary=_is_binary(x), logical=_is_logical(x) or bool(getattr(x, "r_logical", False)))


# ----------------------------------------------------------------------------------------------- dimnames
def concat_dimname(nm1, nm2, nrow1, nrow2):
    """R/rbind.R:136-152"""
    if nm1 is None and nm2 is None:
        return None
    if nm1 is None:
        nm1 = [""] * nrow1
    if nm2 is None:
        nm2 = [""] * nrow2
    return list(nm1) + list(nm2)


def concat_dimnames(mat1, mat2):
    """R/rbind.R:154-186.  :163 is kept as written: with column names on mat1 only and fewer columns than mat2 it
    asks rep() for a negative count, which is R's error."""
    dn1, dn2 = dimnames_of(mat1), dimnames_of(mat2)
    dim1 = concat_dimname(dn1[0], dn2[0], mat1.Dim[0], mat2.Dim[0])
    if dn1[1] is not None:
        dim2 = list(dn1[1])
        if mat1.Dim[1] < mat2.Dim[1]:
            if dn2[1] is not None:
                dim2 = dim2 + list(dn2[1])[len(dim2):]
            elif len(dim2) > 0:
                stop("invalid 'times' argument")
    elif dn2[1] is not None:
        dim2 = list(dn2[1])
    else:
        dim2 = None
    return [dim1, dim2]


def _cbind_dimnames(x, y):
    """R/cbind.R:107-130; :123 tests x's column names twice, as written, so y's may be missing from the result"""
    dnx, dny = dimnames_of(x), dimnames_of(y)
    nx, ny = x.Dim[0], y.Dim[0]
    out = [None, None]
    if dnx[0] is not None:
        out[0] = list(dnx[0])
        if nx < ny:
            out[0] += [""] * (ny - nx) if dny[0] is None else list(dny[0])[:ny - nx]
    elif dny[0] is not None:
        out[0] = list(dny[0])
        if ny < nx:
            out[0] += [""] * (nx - ny)
    if dnx[1] is not None:                                                # :123-126
        out[1] = list(dnx[1]) + (list(dny[1]) if dny[1] is not None else [])
    elif dny[1] is not None:
        out[1] = [""] * x.Dim[1] + list(dny[1])
    return out


# ----------------------------------------------------------------------------------------------- rbind_csr
def rbind_csr(*args):
    """rbind_csr (R/rbind.R:25-114): any number of CSR matrices and sparse vectors (other classes are converted)
    bound by rows into one dgRMatrix / lgRMatrix / ngRMatrix by ONE batched device concat.  Column names are not
    kept."""
    def cast_if_not_csr(x):                                               # :30-41
        if isinstance(x, RsparseMatrix):
            check_valid_matrix(x)
            return x
        if isinstance(x, sparseVector):
            return x
        if _is_dense_vector(x):                                           # a dense vector is one row; logical stays so
            v = _dense_as_svec(x)
            if _dense_dtype(x)[1] == MX_LGL:
                lx = np.where(np.isnan(v.x), NA_LOGICAL, (v.x != 0).astype(np.int32)).astype(np.int32)
                return lsparseVector(v.i, lx, v.length)
            return v
        # a triangular with diag = "N" passes through unexpanded (:31-34): its slots are the general CSR already,
        # and _cast_csr_same relabels them without a copy; every other structured class is expanded
        return _cast_csr_same(x)

    args = [cast_if_not_csr(x) for x in args]
    ncols = max([_ncol(x) for x in args], default=0)                      # :43
    args = [x for x in args if isinstance(x, sparseVector) or x.Dim[0] > 0]          # :45-54
    if len(args) == 0:                                                    # :56-59
        return dgRMatrix(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), (0, ncols))
    if len(args) == 1:                                                    # :60-61
        return _cast_csr_same(args[0])
    if len(args) == 2:                                                    # :62-63
        return rbind2(args[0], args[1])

    is_numeric = [not _is_binary(x) and not _is_logical(x) for x in args]            # :66-75
    kind = "d" if any(is_numeric) else "l" if any(_is_logical(x) for x in args) else "n"
    nrows = sum(_nrow(x) for x in args)                                   # :77-83
    nnz = sum(x.i.size if isinstance(x, sparseVector) else x.j.size for x in args)
    if nrows >= _INT_MAX:
        stop("Result has too many rows for R to handle.")
    if nnz >= _INT_MAX:
        stop("Result has too many non-zero entries for R to handle.")
    cls = _CSR_OF_KIND[kind]
    if not nrows or not ncols:                                            # :94-95
        return cls(np.zeros(nrows + 1, np.int32), np.zeros(nnz, np.int32),
                   None if kind == "n" else np.zeros(nnz, cls.value_dtype), (nrows, ncols))
    res = exports.concat_csr_batch([_row_operand(x) for x in args], _OUT[kind])      # :97
    out = cls(res["indptr"], res["indices"], res["values"], (nrows, ncols))
    if any(not isinstance(x, sparseVector) and dimnames_of(x)[0] is not None for x in args):     # :99-111
        names = []
        for x in args:
            own = None if isinstance(x, sparseVector) else dimnames_of(x)[0]
            names += [str(n) for n in own] if own is not None else [""] * _nrow(x)
        out.Dimnames = [names, None]
    return out


# ----------------------------------------------------------------------------------------------- rbind2
def _rbind2_rows(x, y):
    """rbind2 of RsparseMatrix / sparseVector / CsparseMatrix / TsparseMatrix operands that is neither C-C nor COO:
    rbind2_generic's zero-row shortcuts (:254-265), the kind rule (:311-317) and concat_dimnames, as a two-operand
    batch"""
    if not isinstance(x, sparseVector) and x.Dim[0] <= 0:                 # :254-259
        y = _svec_as_row(y) if isinstance(y, sparseVector) else y
        return _with_dim(y, (y.Dim[0], max(y.Dim[1], x.Dim[1])))
    if not isinstance(y, sparseVector) and y.Dim[0] <= 0:                 # :260-265
        x = _svec_as_row(x) if isinstance(x, sparseVector) else x
        return _with_dim(x, (x.Dim[0], max(x.Dim[1], y.Dim[1])))
    kind = _kind2(x, y)
    ops = []
    for o in (x, y):
        if not isinstance(o, (RsparseMatrix, sparseVector)):              # :297-300
            o = as_csr_matrix(o, logical=_is_logical(o), binary=_is_binary(o))
        if isinstance(o, RsparseMatrix):
            check_valid_matrix(o)                                         # :201-202
        ops.append(o)
    nrows, ncols = _nrow(ops[0]) + _nrow(ops[1]), max(_ncol(ops[0]), _ncol(ops[1]))
    if nrows >= _INT_MAX:                                                 # :204-205, message as written
        stop("Resulting matrix has too many rows for R to handle.")
    res = exports.concat_csr_batch([_row_operand(o) for o in ops], _OUT[kind])
    out = _CSR_OF_KIND[kind](res["indptr"], res["indices"], res["values"], (nrows, ncols))
    mats = [o if isinstance(o, RsparseMatrix) else RsparseMatrix(np.zeros(2, np.int32), np.zeros(0, np.int32), None,
                                                                 (1, o.length)) for o in ops]
    out.Dimnames = concat_dimnames(mats[0], mats[1])
    return out


def _coo_operand(x):
    kind = 0 if isinstance(x, dgTMatrix) else 1 if isinstance(x, lgTMatrix) else 2
    return (kind, x.i, x.j, x.x, x.Dim[0])


def rbind2_coo(x, y):
    """R/rbind.R:405-462: two TsparseMatrix operands, the triplets of x and then those of y moved down"""
    if x.Dim[0] <= 0:                                                     # :407-412
        return _with_dim(y, (y.Dim[0], max(y.Dim[1], x.Dim[1])))
    if y.Dim[0] <= 0:                                                     # :413-418
        return _with_dim(x, (x.Dim[0], max(x.Dim[1], y.Dim[1])))
    check_valid_matrix(x)
    check_valid_matrix(y)
    kind = _kind2(x, y)                                                   # :430-436
    res = exports.rbind_coo([_coo_operand(x), _coo_operand(y)], _OUT[kind])
    out = _COO_OF_KIND[kind](res["ii"], res["jj"], res["xx"], (x.Dim[0] + y.Dim[0], max(x.Dim[1], y.Dim[1])))
    out.Dimnames = concat_dimnames(x, y)                                  # :439
    return out


def rbind2_coo_vec(x, v, x_is_first):
    """R/rbind.R:468-520: the matrix's triplets are stored first either way; with the vector first they move down by
    one and the vector is row 0.  No dimnames (:492 sets Dim alone)."""
    if x.Dim[0] <= 0:                                                     # :470-474
        v = _svec_as_row(v)
        return _with_dim(v, (v.Dim[0], max(v.Dim[1], x.Dim[1])))
    check_valid_matrix(x)
    kind = _kind2(x, v)                                                   # :484-490
    offsets = [0, x.Dim[0]] if x_is_first else [1, 0]                     # :493-499
    res = exports.rbind_coo([_coo_operand(x), (_svec_kind(v), None, v.i, v.x, 1)], _OUT[kind], row_offsets=offsets)
    return _COO_OF_KIND[kind](res["ii"], res["jj"], res["xx"], (x.Dim[0] + 1, max(x.Dim[1], v.length)))


def _no_method(what, x, y):
    raise MatrixExtraError(f"{what}: no method for ({type(x).__name__}, {type(y).__name__}).")


def rbind2(x, y):
    """The rbind2 methods of R/rbind.R:322-401, :466, :524-542 by the classes of x and y."""
    x, y = _expanded(x), _expanded(y)
    xd, yd = _is_dense_vector(x), _is_dense_vector(y)
    if xd or yd:
        if xd and yd:
            _no_method("rbind2", x, y)
        m = y if xd else x
        if isinstance(m, dgCMatrix):                                      # the result stays a CSC
            mt = t_shallow(m)
            return t_shallow(cbind2(x, mt) if xd else cbind2(mt, y))
        if not isinstance(m, RsparseMatrix):                              # a TsparseMatrix has no such method
            _no_method("rbind2", x, y)
        check_valid_matrix(m)
        v = _dense_as_svec(x if xd else y, m.Dim[1], "rbind2")
        ops = [v, m] if xd else [m, v]
        res = exports.concat_csr_batch([_row_operand(o) for o in ops], 0)
        out = dgRMatrix(res["indptr"], res["indices"], res["values"], (m.Dim[0] + 1, m.Dim[1]))
        dn = dimnames_of(m)
        rows = None if dn[0] is None else ([""] + list(dn[0]) if xd else list(dn[0]) + [""])
        out.Dimnames = [rows, None if dn[1] is None else list(dn[1])]
        return out
    xT, yT = isinstance(x, TsparseMatrix), isinstance(y, TsparseMatrix)
    xC, yC = isinstance(x, dgCMatrix), isinstance(y, dgCMatrix)
    xv, yv = isinstance(x, sparseVector), isinstance(y, sparseVector)
    known = (RsparseMatrix, TsparseMatrix, dgCMatrix, sparseVector)
    if not isinstance(x, known) or not isinstance(y, known):
        _no_method("rbind2", x, y)
    if xT and yT:                                                         # :466
        return rbind2_coo(x, y)
    if xT and yv:                                                         # :524
        return rbind2_coo_vec(x, y, True)
    if xv and yT:                                                         # :528
        return rbind2_coo_vec(y, x, False)
    if (xT and yC) or (xC and yT):                                        # :532-542
        if xC:
            x = as_coo_matrix(x)
        else:
            y = as_coo_matrix(y)
        return rbind2_coo(x, y)
    if xC and yC:                                                         # :279-280
        check_valid_matrix(x)
        check_valid_matrix(y)
        return t_shallow(cbind_csr(t_shallow(x), t_shallow(y)))
    return _rbind2_rows(x, y)


# ----------------------------------------------------------------------------------------------- cbind
def _svec_as_col(v):
    """as(v, "RsparseMatrix") of a sparse vector in cbind: one column, through the device cbind with an empty matrix"""
    kind = "n" if _is_binary(v) else "l" if _is_logical(v) else "d"
    empty = np.zeros(1, np.int32), np.zeros(0, np.int32)
    res = exports.cbind_csr_svec(empty[0], empty[1], None, 0, 2, v.i, v.x, _svec_kind(v), v.length, False, _OUT[kind])
    return _CSR_OF_KIND[kind](res["indptr"], res["indices"], res["values"], (v.length, 1))


def cbind_csr(x, y):
    """cbind_csr (R/cbind.R:57-133): two CSR matrices side by side; a TsparseMatrix goes through as.csr.matrix
    (:139-146)."""
    x, y = [as_csr_matrix(o, logical=_is_logical(o), binary=_is_binary(o)) if isinstance(o, TsparseMatrix) else o
            for o in (x, y)]
    if not isinstance(x, sparseVector) and x.Dim[1] <= 0:                 # :59-64
        y = _svec_as_col(y) if isinstance(y, sparseVector) else y
        return _with_dim(y, (max(y.Dim[0], x.Dim[0]), y.Dim[1]))
    if not isinstance(y, sparseVector) and y.Dim[1] <= 0:                 # :65-70
        x = _svec_as_col(x) if isinstance(x, sparseVector) else x
        return _with_dim(x, (max(x.Dim[0], y.Dim[0]), x.Dim[1]))
    if not isinstance(x, RsparseMatrix) or not isinstance(y, RsparseMatrix):
        stop(_INTERNAL_ERROR)
    check_valid_matrix(x)                                                 # :72-73
    check_valid_matrix(y)
    kind = _kind2(x, y)                                                   # :82-99
    ncx = x.Dim[1]
    if ncx + y.Dim[1] > _INT_MAX:
        stop("Resulting matrix has too many columns for R to handle.")
    if kind == "n":
        res = exports.cbind_csr_binary(x.p, x.j, y.p, y.j + np.int32(ncx))
    elif kind == "l":
        xl, yl = as_csr_matrix(x, logical=True), as_csr_matrix(y, logical=True)
        res = exports.cbind_csr_logical(xl.p, xl.j, xl.x, yl.p, yl.j + np.int32(ncx), yl.x)
    else:
        xd, yd = as_csr_matrix(x), as_csr_matrix(y)
        res = exports.cbind_csr_numeric(xd.p, xd.j, xd.x, yd.p, yd.j + np.int32(ncx), yd.x)
    out = _CSR_OF_KIND[kind](res["indptr"], res["indices"], None if kind == "n" else res["values"],
                             (max(x.Dim[0], y.Dim[0]), ncx + y.Dim[1]))      # :101-105
    out.Dimnames = _cbind_dimnames(x, y)
    return out


def _cbind_csr_svec(X, v, first, kind=None):
    """cbind2(RsparseMatrix, sparseVector) (first=False) and cbind2(sparseVector, RsparseMatrix) (first=True) on the
    device: the vector is one more column; max(nrow, length) rows.  The export refuses indices outside 1..length
    (the reference's check_valid_svec would refuse a vector whose last position is stored)."""
    check_valid_matrix(X)
    kind = kind or (_kind2(v, X) if first else _kind2(X, v))
    if X.Dim[1] + 1 > _INT_MAX:
        stop("Resulting matrix has too many columns for R to handle.")
    res = exports.cbind_csr_svec(X.p, X.j, X.x, X.Dim[1], _csr_kind(X), v.i, v.x, _svec_kind(v), v.length, first,
                                 _OUT[kind])
    nrows = max(X.Dim[0], v.length)
    out = _CSR_OF_KIND[kind](res["indptr"], res["indices"], res["values"], (nrows, X.Dim[1] + 1))
    dn = dimnames_of(X)
    rows = None if dn[0] is None else list(dn[0]) + [""] * (nrows - X.Dim[0])
    cols = None if dn[1] is None else ([""] + list(dn[1]) if first else list(dn[1]) + [""])
    out.Dimnames = [rows, cols]
    return out


def cbind2(x, y):
    """The cbind2 methods of R/cbind.R:20-54, :137, :150-195 by the classes of x and y."""
    x, y = _expanded(x), _expanded(y)
    xd, yd = _is_dense_vector(x), _is_dense_vector(y)
    if xd or yd:
        if xd and yd:
            _no_method("cbind2", x, y)
        m = y if xd else x
        if isinstance(m, dgCMatrix):                                      # the result stays a CSC
            mt = t_shallow(m)
            return t_shallow(rbind2(x, mt) if xd else rbind2(mt, y))
        if not isinstance(m, RsparseMatrix):
            _no_method("cbind2", x, y)
        v = _dense_as_svec(x if xd else y, m.Dim[0], "cbind2")
        return _cbind_csr_svec(m, v, first=xd, kind="d")
    xT, yT = isinstance(x, TsparseMatrix), isinstance(y, TsparseMatrix)
    xC, yC = isinstance(x, dgCMatrix), isinstance(y, dgCMatrix)
    xv, yv = isinstance(x, sparseVector), isinstance(y, sparseVector)
    xR, yR = isinstance(x, RsparseMatrix), isinstance(y, RsparseMatrix)
    if xT and yT:                                                         # :20-22
        return t_shallow(rbind2_coo(t_shallow(x), t_shallow(y)))
    if xT and yv:                                                         # :26-28
        return t_shallow(rbind2_coo_vec(t_shallow(x), y, True))
    if xv and yT:                                                         # :32-34
        return t_shallow(rbind2_coo_vec(t_shallow(y), x, False))
    if xC and yv:                                                         # :38-41
        check_valid_matrix(x)
        return t_shallow(_rbind2_rows(t_shallow(x), y))
    if xv and yC:                                                         # :45-48
        check_valid_matrix(y)
        return t_shallow(_rbind2_rows(x, t_shallow(y)))
    if xv and yv:                                                         # :52-54; numeric, so that a CSC class exists
        return t_shallow(as_csr_matrix(_rbind2_rows(x, y)))
    if xC and yC:
        check_valid_matrix(x)
        check_valid_matrix(y)
        return t_shallow(_rbind2_rows(t_shallow(x), t_shallow(y)))
    if (xR or xT) and (yR or yT):                                         # :137, :150-154
        return cbind_csr(x, y)
    if xR and yv:                                                         # :178
        return _cbind_csr_svec(x, y, first=False)
    if xv and yR:                                                         # :195
        return _cbind_csr_svec(y, x, first=True)
    _no_method("cbind2", x, y)


def rbind(*args):
    """rbind(...) as R dispatches it: a left fold of rbind2."""
    return functools.reduce(rbind2, args) if args else None


def cbind(*args):
    """cbind(...) as R dispatches it: a left fold of cbind2."""
    return functools.reduce(cbind2, args) if args else None
