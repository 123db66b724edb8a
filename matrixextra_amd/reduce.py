"""Mirror of the reductions of a sparse matrix: rowSums / colSums / rowMeans / colMeans, norm and diag.

norm and diag are MatrixExtra's own methods for an RsparseMatrix (R/csr_linalg.R: norm_csr :13-31, diag_csr :41-43);
the margin functions are Matrix's, which the vignette's gradient needs on the product it has just made
(colMeans(X * v), vignettes/Introducing_MatrixExtra.Rmd:454-470).  All of them run on the device through the export
level of include/mxgpu_reduce.h (segmented reduction over entries); nothing here computes.

Operands: dgRMatrix / lgRMatrix / ngRMatrix; a dgCMatrix, whose (p, i, x) are the CSR slots of its transpose, so the
same routines serve it with the axes swapped; a TsparseMatrix, through as_csr_matrix, which merges repeated triplets
first, as Matrix's reductions see them.  A logical matrix counts TRUE as 1, a stored FALSE as 0 and NA as NA; a
pattern matrix counts every entry as 1.

Not mirrored: `diag(x) <- value`, norm(type = "2"), and the sparseResult / dims arguments of Matrix's margin
functions.
"""
from __future__ import annotations

import numpy as np

from . import _lib, exports
from .matrices import (MatrixExtraError, RsparseMatrix, TsparseMatrix, as_csr_matrix, check_valid_matrix, dgCMatrix,
                       dimnames_of, lgRMatrix, stop)
from .structured import StructuredMatrix

NORM_TYPES = ("O", "o", "1", "I", "i", "F", "f", "M", "m", "2")
_NORM_KIND = {"O": "O", "o": "O", "1": "O", "I": "I", "i": "I", "F": "F", "f": "F", "M": "M", "m": "M"}


class NamedVector(np.ndarray):
    """A base-R vector with a `names` attribute (None when it has none): what the margin functions return."""

    def __new__(cls, data, names=None):
        obj = np.asarray(data).view(cls)
        obj.names = None if names is None else list(names)
        return obj

    def __array_finalize__(self, obj):
        self.names = getattr(obj, "names", None)


def _operand(x):
    """(p, idx, values, value_dtype, nrow, ncol of the CSR that the slots form, transposed?, Dimnames of x)"""
    if isinstance(x, (TsparseMatrix, StructuredMatrix)):
        x = as_csr_matrix(x)                    # validates; sorts and merges repeated triplets, or expands, on the device
    if isinstance(x, dgCMatrix):
        check_valid_matrix(x)
        return x.p, x.i, x.x, _lib.MX_F64, x.Dim[1], x.Dim[0], True, dimnames_of(x)
    if not isinstance(x, RsparseMatrix):
        stop("Reductions take an RsparseMatrix, a dgCMatrix or a TsparseMatrix.")
    check_valid_matrix(x)
    vd = _lib.MX_NONE if x.x is None else _lib.MX_LGL if isinstance(x, lgRMatrix) else _lib.MX_F64
    return x.p, x.j, x.x, vd, x.Dim[0], x.Dim[1], False, dimnames_of(x)


def _margin(x, over_rows, na_rm, mean):
    """one result per row (over_rows) or per column of x, named by that dimension's names"""
    p, idx, vals, vd, nrow, ncol, transposed, names = _operand(x)
    axis = 0 if over_rows != transposed else 1          # the rows of a CSC are the columns of its CSR slots
    res = exports.csr_margin_reduce(p, idx, vals, ncol, axis, _lib.MX_RED_SUM, bool(na_rm), mean, value_dtype=vd)
    return NamedVector(res, names[0 if over_rows else 1])


def rowSums(x, na_rm=False):
    """rowSums(x, na.rm): a numeric vector with one sum per row, named by the row names."""
    return _margin(x, True, na_rm, False)


def colSums(x, na_rm=False):
    """colSums(x, na.rm): one sum per column, named by the column names."""
    return _margin(x, False, na_rm, False)


def rowMeans(x, na_rm=False):
    """rowMeans(x, na.rm): each row's sum over ncol(x); with na_rm over ncol(x) less the NAs skipped in that row
    (cells that are not stored are zeros, not NAs; a row of nothing but NAs gives NaN)."""
    return _margin(x, True, na_rm, True)


def colMeans(x, na_rm=False):
    """colMeans(x, na.rm): each column's sum over nrow(x), less the NAs skipped in that column with na_rm."""
    return _margin(x, False, na_rm, True)


def norm(x, type="O"):
    """norm(x, type) — norm_csr, R/csr_linalg.R:13-31: "O" / "o" / "1" the largest column sum of |x|, "I" / "i" the
    largest row sum, "F" / "f" the Frobenius norm, "M" / "m" the largest |x|.  "2" is allowed by the reference and
    handed on to Matrix's spectral norm, which has no counterpart here: it raises MatrixExtraError.  An operand
    without entries or with a zero dimension has norm 0; any NaN / NA that contributes makes the result NaN."""
    if isinstance(type, (list, tuple, np.ndarray)):
        if len(type) == 0 or not all(isinstance(t, str) for t in type):
            stop("'type' must be a single character variable (see ?norm).")
        type = type[0]
    if not isinstance(type, str):
        stop("'type' must be a single character variable (see ?norm).")
    if type not in NORM_TYPES:
        stop("Invalid norm type. Allowed values: " + ", ".join(NORM_TYPES))
    if type == "2":
        raise MatrixExtraError("norm(type = \"2\") is the spectral norm, which stays with Matrix: it is not computed "
                               "on the device.")
    p, idx, vals, vd, nrow, ncol, transposed, _ = _operand(x)
    kind = _NORM_KIND[type]
    if transposed and kind in ("O", "I"):               # a column of x is a row of the slots' CSR
        kind = "I" if kind == "O" else "O"
    return exports.csr_norm(p, idx, vals, ncol, kind, value_dtype=vd)


def diag(x):
    """diag(x) — diag_csr, R/csr_linalg.R:41-43: the main diagonal as a vector of min(dim(x)) values, numeric for a
    numeric matrix, int32 R logicals (NA kept) for a logical one and for a pattern matrix (0 / 1).  Cells that are
    not stored give 0."""
    p, idx, vals, vd, nrow, ncol, _, _ = _operand(x)    # the diagonal of the transpose is the same diagonal
    return exports.csr_diag(p, idx, vals, ncol, value_dtype=vd)
