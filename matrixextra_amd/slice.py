"""Host-side mirror of the row-selection part of R/slice.R (`X[i, ]`).

`subset_csr(x, i, j)` takes R-style indices: 1-based integers (repeats allowed),
negative integers = exclusion, logical masks (recycled like base R), dimnames.
Path selection follows R/slice.R:439-565: a contiguous ascending run of rows with
all columns is sliced on the host exactly as the reference does in pure R
(:477-483, never reaches native code there either); everything else goes to the
native routines — row gather, column-range / arbitrary-column slices, reversals.

`subset_coo(x, i, j, drop)` is the same for a TsparseMatrix, after R/slice_coo.R: a scalar (i, j) pair goes to
slice_coo_single_*, everything else to slice_coo_arbitrary_* (the COO slice kernels).
"""
from __future__ import annotations

import numpy as np

from . import exports
from .matrices import (RsparseMatrix, TsparseMatrix, check_valid_matrix, dgRMatrix, dgTMatrix, lgRMatrix,
                       lgTMatrix, ngRMatrix, ngTMatrix, stop)


def get_indices_integer(i, max_i, index_names):
    """R/slice.R:2-53 for integer / logical / character `i`; returns 1-based int32."""
    i = np.asarray(i)
    if i.dtype.kind in ("U", "S", "O"):
        if index_names is not None:
            lookup = {nm: k + 1 for k, nm in reversed(list(enumerate(index_names)))}
            try:
                i = np.array([lookup[s] for s in i.tolist()], dtype=np.int64)
            except KeyError:
                stop("some of row subset indices are not present in matrix")
        else:
            i = i.astype(np.int64)
    if i.dtype == np.bool_:
        if i.size != max_i:
            if i.size > max_i:
                stop("some of row subset indices are not present in matrix")
            reps = -(-max_i // max(i.size, 1))
            i = np.tile(i, reps)[:max_i]            # seq(1, max_i)[i] recycles the mask
        i = np.flatnonzero(i) + 1
    i = i.astype(np.int64, copy=False).reshape(-1)
    if np.any(i <= 0):
        if np.any(i > 0):
            stop("can't mix positive and negative subscripts")
        keep = np.ones(max_i, dtype=bool)
        drop = -i[i < 0]
        if np.any(drop > max_i):
            drop = drop[drop <= max_i]
        keep[drop - 1] = False
        i = np.flatnonzero(keep) + 1
    if i.size and np.any(i > max_i):
        stop("some of row subset indices are not present in matrix")
    return i.astype(np.int32)


class IJProperties:
    """What get_ij_properties returns (R/slice.R:59-143), without the NA fields: 1-based int32 `i` / `j`, the six
    classification flags, n_row / n_col, and the selected dimnames (None when the matrix has none)."""
    __slots__ = ("i", "j", "all_i", "all_j", "i_is_seq", "j_is_seq", "i_is_rev_seq", "j_is_rev_seq", "n_row",
                 "n_col", "row_names", "col_names")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def get_ij_properties(x, i, j):
    """R/slice.R:59-143 for integer / logical / name / negative selectors (`None` = missing).  The asymmetry is the
    reference's (:79-103): a full-range i sets both all_i and i_is_seq, a full-range j sets all_j and leaves
    j_is_seq FALSE."""
    row_names, col_names = x.Dimnames[0], x.Dimnames[1]
    nrow, ncol = x.Dim
    all_i = all_j = i_is_seq = j_is_seq = i_is_rev_seq = j_is_rev_seq = False
    if j is None:
        all_j = True
        j = np.arange(1, ncol + 1, dtype=np.int32)
    else:
        j = get_indices_integer(j, ncol, col_names)
        if j.size == ncol and ncol > 0 and j[0] == 1 and j[-1] == ncol:
            all_j = exports.check_is_seq(j)
        else:
            j_is_seq = exports.check_is_seq(j)
    if i is None:
        i = np.arange(1, nrow + 1, dtype=np.int32)
        all_i = i_is_seq = True
    else:
        i = get_indices_integer(i, nrow, row_names)
        i_is_seq = exports.check_is_seq(i)
        if i_is_seq and i.size == nrow and nrow > 0 and i[0] == 1 and i[-1] == nrow:
            all_i = True
    if not all_i and not i_is_seq:
        i_is_rev_seq = exports.check_is_rev_seq(i)
    if not all_j and not j_is_seq:
        j_is_rev_seq = exports.check_is_rev_seq(j)
    new_rn = None if row_names is None or not len(row_names) else [row_names[k - 1] for k in i]
    new_cn = None if col_names is None or not len(col_names) else [col_names[k - 1] for k in j]
    return IJProperties(i=i, j=j, all_i=all_i, all_j=all_j, i_is_seq=i_is_seq, j_is_seq=j_is_seq,
                        i_is_rev_seq=i_is_rev_seq, j_is_rev_seq=j_is_rev_seq, n_row=int(i.size), n_col=int(j.size),
                        row_names=new_rn, col_names=new_cn)


def _empty_like(x, n_row, row_names):
    cls = dgRMatrix if isinstance(x, dgRMatrix) else lgRMatrix if isinstance(x, lgRMatrix) else ngRMatrix
    xv = None if cls is ngRMatrix else np.zeros(0, dtype=cls.value_dtype)
    return cls(np.zeros(n_row + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), xv,
               (n_row, x.Dim[1]), [row_names, x.Dimnames[1]])


def _cls_kind(x):
    return "d" if isinstance(x, dgRMatrix) else "l" if isinstance(x, lgRMatrix) else "n"


def _call3(kind, fn_numeric, fn_logical, fn_binary, p, j, xv, *rest):
    if kind == "d":
        return fn_numeric(p, j, xv, *rest)
    if kind == "l":
        return fn_logical(p, j, xv, *rest)
    return fn_binary(p, j, *rest)


def subset_csr(x, i=None, j=None, drop=False):
    """`x[i, j]` for RsparseMatrix — R/slice.R:293-585 (integer / logical / name / negative indices; NA indices and
    `drop` to vectors are not mirrored).  Branch selection is the reference's (:439-565):
      contiguous ascending rows, all columns      -> host slicing, as the reference does in pure R (:477-483)
      descending rows, all columns                -> host slicing + reverse_rows_*                    (:484-501)
      other rows, all columns                     -> copy_csr_rows_*            (row-gather kernel)   (:502-515)
      contiguous ascending columns                -> copy_csr_rows_col_seq_*                          (:516-529)
      contiguous descending columns               -> copy_csr_rows_col_seq_* + reverse_columns_inplace_* (:530-546)
      anything else                               -> copy_csr_arbitrary_*                             (:547-565)
      full reversal of both                       -> reverse_rows_* + reverse_columns_inplace_*       (:439-469)"""
    check_valid_matrix(x)
    if i is None and j is None:
        return x
    P = get_ij_properties(x, i, j)
    i, j = P.i, P.j
    nrow, ncol = x.Dim
    all_i, all_j, i_is_seq, j_is_seq = P.all_i, P.all_j, P.i_is_seq, P.j_is_seq
    i_is_rev_seq, j_is_rev_seq = P.i_is_rev_seq, P.j_is_rev_seq
    n_row, n_col = P.n_row, P.n_col
    new_rn, new_cn = P.row_names, P.col_names

    if n_row == 0 or n_col == 0 or x.j.size == 0:              # R/slice.R:404-421
        out = _empty_like(x, n_row, new_rn)
        out.Dim = (n_row, n_col)
        out.Dimnames = [new_rn, new_cn]
        return out
    if all_i and all_j:                                         # R/slice.R:423-425
        return x

    kind = _cls_kind(x)
    has_x = x.x is not None
    E = exports

    def finish(indptr, col_indices, x_values):
        res = type(x).__new__(type(x))                          # new(class(x)[1L])  R/slice.R:567
        res.p = indptr
        res.j = col_indices
        if has_x:                                               # res@x <- as.logical(x_values) for lsparse (:571-575)
            if kind == "l" and x_values is not None and x_values.dtype != np.int32:
                x_values = np.where(np.isnan(x_values), np.int32(-2147483648), (x_values != 0)).astype(np.int32)
            res.x = x_values
        else:
            res.x = None
        res.Dim = (n_row, n_col)
        res.Dimnames = [new_rn, new_cn]
        return res

    if i_is_rev_seq and j_is_rev_seq and n_row == nrow and n_col == ncol:          # R/slice.R:439-469
        t = _call3(kind, E.reverse_rows_numeric, E.reverse_rows_logical, E.reverse_rows_binary, x.p, x.j, x.x)
        jj = np.ascontiguousarray(t["indices"])
        xx = np.ascontiguousarray(t["values"]) if has_x else None
        if kind == "d":
            E.reverse_columns_inplace_numeric(t["indptr"], jj, xx, ncol)
        elif kind == "l":
            E.reverse_columns_inplace_logical(t["indptr"], jj, xx, ncol)
        else:
            E.reverse_columns_inplace_binary(t["indptr"], jj, ncol)
        return finish(t["indptr"], jj, xx)

    if i_is_seq and all_j:                                      # R/slice.R:477-483 (pure R in the reference too)
        first, last = int(x.p[i[0] - 1]), int(x.p[i[-1]])
        return finish(x.p[i[0] - 1:i[-1] + 1] - x.p[i[0] - 1], x.j[first:last], x.x[first:last] if has_x else None)
    if i_is_rev_seq and all_j:                                  # R/slice.R:484-501
        first, last = int(x.p[i[-1] - 1]), int(x.p[i[0]])
        indptr = (x.p[i[-1] - 1:i[0] + 1] - x.p[i[-1] - 1]).astype(np.int32)
        t = _call3(kind, E.reverse_rows_numeric, E.reverse_rows_logical, E.reverse_rows_binary,
                   indptr, x.j[first:last], x.x[first:last] if has_x else None)
        return finish(t["indptr"], t["indices"], t["values"] if has_x else None)
    rows0 = (i - 1).astype(np.int32)
    if all_j:                                                   # R/slice.R:502-515 -> gather kernel
        t = _call3(kind, E.copy_csr_rows_numeric, E.copy_csr_rows_logical, E.copy_csr_rows_binary, x.p, x.j, x.x, rows0)
        return finish(t["indptr"], t["indices"], t["values"] if has_x else None)
    if j_is_seq or j_is_rev_seq:                                # R/slice.R:516-546
        t = _call3(kind, E.copy_csr_rows_col_seq_numeric, E.copy_csr_rows_col_seq_logical,
                   E.copy_csr_rows_col_seq_binary, x.p, x.j, x.x, rows0, j, True)
        jj = np.ascontiguousarray(t["indices"])
        xx = np.ascontiguousarray(t["values"]) if has_x else None
        if j_is_rev_seq:
            new_ncol = int(j[0] - j[-1] + 1)
            if kind == "n":
                E.reverse_columns_inplace_binary(t["indptr"], jj, new_ncol)
            else:                                               # values are numeric here in both classes (slice.cpp:363)
                E.reverse_columns_inplace_numeric(t["indptr"], jj, xx if xx is not None and xx.size else None, new_ncol)
        return finish(t["indptr"], jj, xx)
    t = _call3(kind, E.copy_csr_arbitrary_numeric, E.copy_csr_arbitrary_logical, E.copy_csr_arbitrary_binary,
               x.p, x.j, x.x, rows0, (j - 1).astype(np.int32))  # R/slice.R:547-565
    return finish(t["indptr"], t["indices"], t.get("values") if has_x else None)


def canonical_key(x, key):
    """Python-style key of `X[rows]` / `X[rows, cols]` (0-based, negative = from the end, bool masks, slices) ->
    (rows, cols) as 1-based int32 selectors, None where the whole axis is taken."""
    def canon(k, n):
        if isinstance(k, slice):
            if k == slice(None):
                return None
            return np.arange(n)[k]
        a = np.asarray(k)
        if a.dtype == np.bool_:
            if a.size != n:
                stop("boolean index has wrong length")
            return np.flatnonzero(a)
        a = a.astype(np.int64).reshape(-1)
        a = np.where(a < 0, a + n, a)
        if a.size and (a.min() < 0 or a.max() >= n):
            stop("some of row subset indices are not present in matrix")
        return a
    kj = None
    if isinstance(key, tuple):
        if len(key) != 2:
            stop("incorrect number of dimensions")
        key, kj = key
    rows, cols = canon(key, x.Dim[0]), canon(kj, x.Dim[1]) if kj is not None else None
    return (None if rows is None else (rows + 1).astype(np.int32),
            None if cols is None else (cols + 1).astype(np.int32))


def getitem_python(x, key):
    """Python-style `X[rows]` / `X[rows, :]` (0-based, negative = from the end, bool masks) on top of subset_csr
    (RsparseMatrix) or subset_coo (TsparseMatrix).  `X[2, 3]` is a 1 x 1 RsparseMatrix; `T[2, 3]` (two integers)
    takes R's scalar route with drop=FALSE, a 1 x 1 TsparseMatrix holding the first matching triplet; any other key
    is passed on as vectors."""
    rows, cols = canonical_key(x, key)
    if isinstance(x, TsparseMatrix):
        if isinstance(key, tuple) and all(isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_))
                                          for k in key):
            return subset_coo(x, rows, cols, drop=False)       # X[i, j, drop=FALSE] with integer scalars
        check_valid_matrix(x)
        return _subset_coo_vectors(x, rows, cols)
    return subset_csr(x, rows, cols)


# ----------------------------------------------------------------------------- COO: R/slice_coo.R
def _coo_kind(x):
    return "d" if isinstance(x, dgTMatrix) else "l" if isinstance(x, lgTMatrix) else "n"


_COO_CLS = {"d": dgTMatrix, "l": lgTMatrix, "n": ngTMatrix}


def _is_scalar_number(v):
    """`NROW(v) == 1L && typeof(v) %in% c("integer", "numeric")` (R/slice_coo.R:10-13) for Python values: one int or
    float, not a bool (a logical) and not a name.  R's typeof() of a double is "double", so strictly only integer
    scalars take this route there; a Python caller writes plain numbers for both, and both are taken here."""
    if isinstance(v, (bool, np.bool_)):
        return False
    if isinstance(v, (int, float, np.integer, np.floating)):
        return True
    a = np.asarray(v) if isinstance(v, (list, tuple, np.ndarray)) else None
    return a is not None and a.size == 1 and a.dtype.kind in ("i", "u", "f")


def _empty_coo(kind, n_row, n_col, row_names, col_names):
    xv = None if kind == "n" else np.zeros(0, dtype=_COO_CLS[kind].value_dtype)
    return _COO_CLS[kind](np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), xv, (n_row, n_col),
                          [row_names, col_names])


def _subset_coo_single(x, i, j, drop):
    """R/slice_coo.R:10-84.  The symmetric / triangular branches (:22-42) have no stand-in class here."""
    i, j = int(np.asarray(i).reshape(-1)[0]), int(np.asarray(j).reshape(-1)[0])   # as.integer(): truncates
    nrow, ncol = x.Dim
    if i > nrow or j > ncol:
        stop("Subscript out of bounds.")
    # (sic) a scalar <= 0 is not an exclusion here: it reaches the native routine as i-1 < 0, finds no triplet and
    # gives 0 / FALSE, as the reference does.
    kind = _coo_kind(x)
    if kind == "d":
        res = exports.slice_coo_single_numeric(x.i, x.j, x.x, i - 1, j - 1)
    elif kind == "l":
        res = exports.slice_coo_single_logical(x.i, x.j, x.x, i - 1, j - 1)
    else:
        res = exports.slice_coo_single_binary(x.i, x.j, i - 1, j - 1)
    if drop:
        return res                              # names(res) <- colnames(x)[j] (:55-56) is not mirrored
    rn = x.Dimnames[0][i - 1] if x.Dimnames[0] is not None and len(x.Dimnames[0]) and i >= 1 else None
    cn = x.Dimnames[1][j - 1] if x.Dimnames[1] is not None and len(x.Dimnames[1]) and j >= 1 else None
    out = _empty_coo(kind, 1, 1, None if rn is None else [rn], None if cn is None else [cn])
    if (isinstance(res, float) and np.isnan(res)) or res != 0:            # :76-83
        out.i = np.zeros(1, dtype=np.int32)
        out.j = np.zeros(1, dtype=np.int32)
        if kind == "d":
            out.x = np.array([res], dtype=np.float64)
        elif kind == "l":
            out.x = np.array([1], dtype=np.int32)                        # as.logical(TRUE)
        # ngT: the entry is kept without an x slot (the reference assigns out@x there, which an ngTMatrix lacks)
    return out


def subset_coo(x, i=None, j=None, drop=True):
    """`x[i, j]` for TsparseMatrix — R/slice_coo.R:1-232 (integer / logical / name / negative indices).  As in
    subset_csr, NA indices and `drop` to a vector for non-scalar selections are not mirrored; `drop` only matters
    for the scalar (i, j) route.  Routes:
      both i and j scalar numbers                 -> slice_coo_single_*, a scalar, or 1 x 1 with drop=False (:10-84)
      empty i or j, or no entries                 -> empty T-matrix of the same kind                      (:108-125)
      all rows and all columns                    -> x itself                                             (:127-129)
      full reversal of both                       -> slice_coo_arbitrary_* with the rev-seq flags; the reference
                                                     flips (nrow-1) - i, (ncol-1) - j in R (:142-154), which the
                                                     kernel's affine reversed axes reproduce bit for bit
      anything else                               -> slice_coo_arbitrary_*                                (:160-196)"""
    check_valid_matrix(x)
    if i is None and j is None:
        return x
    if i is not None and j is not None and _is_scalar_number(i) and _is_scalar_number(j):
        return _subset_coo_single(x, i, j, drop)
    return _subset_coo_vectors(x, i, j)


def _subset_coo_vectors(x, i, j):
    """R/slice_coo.R:87-232: everything but the scalar route."""
    P = get_ij_properties(x, i, j)
    kind = _coo_kind(x)
    if P.n_row == 0 or P.n_col == 0 or x.i.size == 0:                  # :108-125
        return _empty_coo(kind, P.n_row, P.n_col, P.row_names, P.col_names)
    if P.all_i and P.all_j:                                             # :127-129
        return x
    nrow, ncol = x.Dim
    flags = (P.all_i, P.all_j, P.i_is_seq, P.j_is_seq, P.i_is_rev_seq, P.j_is_rev_seq, nrow, ncol)
    if kind == "d":
        t = exports.slice_coo_arbitrary_numeric(x.i, x.j, x.x, P.i, P.j, *flags)
    elif kind == "l":
        t = exports.slice_coo_arbitrary_logical(x.i, x.j, x.x, P.i, P.j, *flags)
    else:
        t = exports.slice_coo_arbitrary_binary(x.i, x.j, P.i, P.j, *flags)
    res = type(x).__new__(type(x))                                      # new(class(x)[1L])  :198
    res.i, res.j, res.x = t["ii"], t["jj"], t["xx"] if kind != "n" else None
    res.Dim = (P.n_row, P.n_col)
    res.Dimnames = [P.row_names, P.col_names]
    return res
