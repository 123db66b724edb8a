"""Host-side mirror of the row-selection part of R/slice.R (`X[i, ]`).

`subset_csr(x, i, j)` takes R-style indices: 1-based integers (repeats allowed),
negative integers = exclusion, logical masks (recycled like base R), dimnames.
Path selection follows R/slice.R:439-565: a contiguous ascending run of rows with
all columns is sliced on the host exactly as the reference does in pure R
(:477-483, never reaches native code there either); everything else goes to the
native routines — row gather, column-range / arbitrary-column slices, reversals.

`subset_coo(x, i, j, drop)` is the same for a TsparseMatrix, after R/slice_coo.R: a scalar (i, j) pair goes to
slice_coo_single_*, everything else to slice_coo_arbitrary_* (the COO slice kernels).

A selector may hold NA (NA_INTEGER, a float nan, None) or be an lsparseVector / nsparseVector mask: get_ij_properties
replaces the NAs by the first index that is none and both routes end in inject_NAs, which makes the NA rows and
columns of the result NA throughout.  `drop` to a vector and the CSR scalar lookup are taken under
options["mxgpu.slice_drop_route"].
"""
from __future__ import annotations

import numpy as np

from . import exports, structured
from .matrices import (NA_INTEGER, NA_LOGICAL, NA_REAL, RsparseMatrix, TsparseMatrix, _coo_to_compressed,
                       as_coo_matrix, as_csr_matrix, as_sparse_vector, check_valid_matrix, dgRMatrix, dgTMatrix,
                       lgRMatrix, lgTMatrix, lsparseVector, ngRMatrix, ngTMatrix, nsparseVector, options,
                       sort_sparse_indices, stop)
from .structured import StructuredMatrix


def _svec_selector(v, max_i):
    """R/slice.R:4-30: an lsparseVector / nsparseVector mask as 1-based indices, recycled over the axis like base R
    (repeat_indices_n_times).  An lsparseVector that stores an NA reads as the dense logical it spells (TRUE selects,
    NA gives an NA index); one without NA selects the positions whose stored value is TRUE."""
    v = sort_sparse_indices(v, copy=not options.get("MatrixExtra.inplace_sort", False))
    if v.length > max_i:
        stop("Dimension of indexing vector is larger than matrix to subset.")
    if v.length == 0:
        return np.zeros(0, dtype=np.int32)
    if isinstance(v, lsparseVector):
        if np.any(v.x == NA_LOGICAL):                                 # seq(1L, max_i)[as.logical(i)]
            dense = np.zeros(v.length, dtype=np.int32)
            dense[v.i.astype(np.int64) - 1] = v.x
            reps = -(-max_i // max(v.length, 1))
            dense = np.tile(dense, reps)[:max_i]
            pos = np.flatnonzero(dense != 0)
            return np.where(dense[pos] == NA_LOGICAL, NA_INTEGER, (pos + 1).astype(np.int32)).astype(np.int32)
        v = nsparseVector(v.i[v.x != 0], None, v.length)
    if v.length == max_i:
        return v.i.astype(np.int32)
    remainder = max_i - v.length * (max_i // v.length)                # i[seq(1L, remainder)]@i: the positions inside it
    return exports.repeat_indices_n_times(v.i, v.i[v.i <= remainder], v.length, max_i)


def _as_integer_with_na(i, index_names):
    """(int64 indices, NA mask) of a selector: NA is NA_INTEGER in an integer array, nan in a float one and None in an
    object array (assign._has_na's reading); names are looked up, floats truncated as as.integer() does."""
    i = np.asarray(i)
    if i.dtype.kind == "O":
        flat = i.reshape(-1).tolist()
        na = np.array([v is None or (isinstance(v, (float, np.floating)) and np.isnan(v)) for v in flat], dtype=bool)
        lookup = None
        if index_names is not None and any(isinstance(v, str) for v in flat):
            lookup = {nm: k + 1 for k, nm in reversed(list(enumerate(index_names)))}
        vals = np.zeros(len(flat), dtype=np.int64)
        for k, v in enumerate(flat):
            if na[k]:
                continue
            if lookup is not None:
                if v not in lookup:
                    stop("some of row subset indices are not present in matrix")
                vals[k] = lookup[v]
            else:
                vals[k] = int(v)
        return vals, na
    if i.dtype.kind in ("U", "S"):
        if index_names is not None:
            lookup = {nm: k + 1 for k, nm in reversed(list(enumerate(index_names)))}
            try:
                i = np.array([lookup[s] for s in i.reshape(-1).tolist()], dtype=np.int64)
            except KeyError:
                stop("some of row subset indices are not present in matrix")
        else:
            i = i.astype(np.int64)
        return i.reshape(-1), np.zeros(i.size, dtype=bool)
    i = i.reshape(-1)
    if i.dtype.kind == "f":
        na = np.isnan(i)
        return np.where(na, 0.0, i).astype(np.int64), na
    na = i == NA_INTEGER if i.dtype.kind == "i" else np.zeros(i.size, dtype=bool)
    return np.where(na, 0, i).astype(np.int64), na


def get_indices_integer(i, max_i, index_names):
    """R/slice.R:2-53 for integer / logical / character / sparseVector `i`; returns 1-based int32, NA_INTEGER where
    the selector holds an NA.  An NA is exempt from the exclusion rule and from the bounds check (:48-51)."""
    if isinstance(i, (lsparseVector, nsparseVector)):
        i = _svec_selector(i, max_i)
    i = np.asarray(i)
    if i.dtype == np.bool_:
        if i.size != max_i:
            if i.size > max_i:
                stop("some of row subset indices are not present in matrix")
            reps = -(-max_i // max(i.size, 1))
            i = np.tile(i, reps)[:max_i]            # seq(1, max_i)[i] recycles the mask
        i = np.flatnonzero(i) + 1
    i, na = _as_integer_with_na(i, index_names)
    good = i[~na]
    if np.any(good <= 0):
        if np.any(good > 0):
            stop("can't mix positive and negative subscripts")
        if na.any():
            stop("can't mix NAs with negative subscripts")
        keep = np.ones(max_i, dtype=bool)
        drop = -i[i < 0]
        if np.any(drop > max_i):
            drop = drop[drop <= max_i]
        keep[drop - 1] = False
        i = np.flatnonzero(keep) + 1
        na = np.zeros(i.size, dtype=bool)
    elif good.size and np.any(good > max_i):
        stop("some of row subset indices are not present in matrix")
    out = i.astype(np.int32)
    out[na] = NA_INTEGER
    return out


def find_first_non_na(i):
    """find_first_non_na (src/slice.cpp): the first index that is not NA, or NA_INTEGER.  A host scan: the selector is
    host data and the scan ends at the first hit."""
    for v in i:
        if v != NA_INTEGER:
            return np.int32(v)
    return NA_INTEGER


class IJProperties:
    """What get_ij_properties returns (R/slice.R:59-143): 1-based int32 `i` / `j` (an NA replaced by the first
    index that is none; all NA_INTEGER when every one is), the six classification flags, n_row / n_col, the selected
    dimnames (None when the matrix has none, or when the whole axis is NA), and per axis has_NA, all_NA and NAs — the
    1-based positions of the NA entries in the selector, or None."""
    __slots__ = ("i", "j", "all_i", "all_j", "i_is_seq", "j_is_seq", "i_is_rev_seq", "j_is_rev_seq", "n_row",
                 "n_col", "row_names", "col_names", "i_has_NA", "i_all_NA", "i_NAs", "j_has_NA", "j_all_NA", "j_NAs")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def _fill_NAs(idx):
    """R/slice.R:111-132 for one axis: (indices with the NAs replaced, all_NA, the 1-based NA positions or None)"""
    first = find_first_non_na(idx)
    if first == NA_INTEGER:
        return idx, True, None
    NAs = (np.flatnonzero(idx == NA_INTEGER) + 1).astype(np.int32)
    return np.where(idx == NA_INTEGER, first, idx).astype(np.int32), False, NAs


def get_ij_properties(x, i, j):
    """R/slice.R:59-143 for integer / logical / name / negative / sparseVector selectors (`None` = missing), NA
    entries included.  The asymmetry is the reference's (:79-103): a full-range i sets both all_i and i_is_seq, a
    full-range j sets all_j and leaves j_is_seq FALSE.  The flag checks are skipped for an axis with NAs."""
    row_names, col_names = x.Dimnames[0], x.Dimnames[1]
    nrow, ncol = x.Dim
    all_i = all_j = i_is_seq = j_is_seq = i_is_rev_seq = j_is_rev_seq = False
    i_has_NA = j_has_NA = i_all_NA = j_all_NA = False
    i_NAs = j_NAs = None
    if j is None:
        all_j = True
        j = np.arange(1, ncol + 1, dtype=np.int32)
    else:
        j = get_indices_integer(j, ncol, col_names)
        j_has_NA = bool(np.any(j == NA_INTEGER))
        if not j_has_NA:
            if j.size == ncol and ncol > 0 and j[0] == 1 and j[-1] == ncol:
                all_j = exports.check_is_seq(j)
            else:
                j_is_seq = exports.check_is_seq(j)
    if i is None:
        i = np.arange(1, nrow + 1, dtype=np.int32)
        all_i = i_is_seq = True
    else:
        i = get_indices_integer(i, nrow, row_names)
        i_has_NA = bool(np.any(i == NA_INTEGER))
        if not i_has_NA:
            i_is_seq = exports.check_is_seq(i)
        if i_is_seq and i.size == nrow and nrow > 0 and i[0] == 1 and i[-1] == nrow:
            all_i = True
    if not all_i and not i_is_seq and not i_has_NA:
        i_is_rev_seq = exports.check_is_rev_seq(i)
    if not all_j and not j_is_seq and not j_has_NA:
        j_is_rev_seq = exports.check_is_rev_seq(j)
    if i_has_NA:
        i, i_all_NA, i_NAs = _fill_NAs(i)
    if j_has_NA:
        j, j_all_NA, j_NAs = _fill_NAs(j)
    new_rn = None if row_names is None or not len(row_names) or i_all_NA else [row_names[k - 1] for k in i]
    new_cn = None if col_names is None or not len(col_names) or j_all_NA else [col_names[k - 1] for k in j]
    return IJProperties(i=i, j=j, all_i=all_i, all_j=all_j, i_is_seq=i_is_seq, j_is_seq=j_is_seq,
                        i_is_rev_seq=i_is_rev_seq, j_is_rev_seq=j_is_rev_seq, n_row=int(i.size), n_col=int(j.size),
                        row_names=new_rn, col_names=new_cn, i_has_NA=i_has_NA, i_all_NA=i_all_NA, i_NAs=i_NAs,
                        j_has_NA=j_has_NA, j_all_NA=j_all_NA, j_NAs=j_NAs)


# ----------------------------------------------------------------------------- inject_NAs / drop_slice: R/slice.R:145-236
def _drop_route():
    """`drop` to vectors and the CSR scalar lookup are taken only under options["mxgpu.slice_drop_route"] (off
    unless set): with it off every call returns what it returned before they existed."""
    return bool(options.get("mxgpu.slice_drop_route", False))


def _is_logical_kind(x):
    return isinstance(x, (lgRMatrix, ngRMatrix, lgTMatrix, ngTMatrix))


def _names_without(names, NAs):
    if names is None or NAs is None or not NAs.size:
        return names
    names = list(names)
    for k in NAs:
        names[k - 1] = None                                            # NA_character_
    return names


def inject_NAs(x, i_NAs, j_NAs):
    """R/slice.R:145-208: rows i_NAs and columns j_NAs (1-based positions in x) become NA throughout; their dimnames
    become None.  A CSR takes two scalar assignments of NA_real_ (§4.16) as a dgRMatrix and goes back to logical for
    lgRMatrix / ngRMatrix input; a COO goes to inject_NAs_inplace_coo_* as a dgTMatrix / lgTMatrix.  The reference
    leaves the COO result without dimnames (it fills a new object, :183-192); here it keeps them."""
    ni = 0 if i_NAs is None else int(i_NAs.size)
    nj = 0 if j_NAs is None else int(j_NAs.size)
    if not ni and not nj:
        return x
    names = [_names_without(x.Dimnames[0], i_NAs), _names_without(x.Dimnames[1], j_NAs)]
    nrow, ncol = x.Dim
    logical = _is_logical_kind(x)
    if isinstance(x, RsparseMatrix):
        from .assign import _assign_csr_internal                      # assign imports this module
        y = as_csr_matrix(x)
        y = dgRMatrix(y.p, y.j, y.x, y.Dim, names)
        if ni:
            y = _assign_csr_internal(y, i_NAs, np.arange(1, ncol + 1, dtype=np.int32), NA_REAL, None)
        if nj:
            y = _assign_csr_internal(y, np.arange(1, nrow + 1, dtype=np.int32), j_NAs, NA_REAL, None)
        return as_csr_matrix(y, logical=True) if logical else y
    y = as_coo_matrix(x, logical=logical)
    rows_na = np.zeros(0, dtype=np.int32) if not ni else (i_NAs - 1).astype(np.int32)
    cols_na = np.zeros(0, dtype=np.int32) if not nj else (j_NAs - 1).astype(np.int32)
    fn = exports.inject_NAs_inplace_coo_logical if logical else exports.inject_NAs_inplace_coo_numeric
    res = fn(y.i, y.j, y.x, rows_na, cols_na, nrow, ncol)
    return (lgTMatrix if logical else dgTMatrix)(res["ii"], res["jj"], res["xx"], x.Dim, names)


def _as_vector(x):
    """as.vector() of a one-row or one-column sparse matrix: float64, or R logicals (int32) for the l and n kinds.  A
    COO goes through the COO -> CSR route first, which merges its repeated triplets."""
    if isinstance(x, TsparseMatrix):
        x = _coo_to_compressed(x)
    nrow, ncol = x.Dim
    pos = x.j if nrow == 1 else np.repeat(np.arange(nrow, dtype=np.int32), np.diff(x.p))
    return exports.entries_to_dense_vector(pos, x.x, nrow * ncol, logical=x.x is None)


def drop_slice(x, drop, i_NAs=None, j_NAs=None):
    """R/slice.R:210-236: inject_NAs, then — under the drop route — a one-row or one-column result as a dense vector,
    or as a sparseVector of its kind under MatrixExtra.drop_sparse when it is not 1 x 1."""
    x = inject_NAs(x, i_NAs, j_NAs)
    if drop and _drop_route() and isinstance(x, (RsparseMatrix, TsparseMatrix)):
        nrow, ncol = x.Dim
        if nrow == 1 or ncol == 1:
            if not (nrow == 1 and ncol == 1) and options.get("MatrixExtra.drop_sparse", False):
                has_x = x.x is not None                                # as(x, "sparseVector") keeps the kind
                return as_sparse_vector(x, binary=not has_x, logical=has_x and x.x.dtype == np.int32)
            return _as_vector(x)
    return x


def _scalar_index(v):
    """as.integer() of a scalar selector, NA_INTEGER for nan / None / NA_INTEGER"""
    v = np.asarray(v, dtype=object).reshape(-1)[0]
    if v is None or (isinstance(v, (float, np.floating)) and np.isnan(v)):
        return int(NA_INTEGER)
    return int(v)


def _na_matrix_entries(n_row, n_col, logical):
    """row-major cells of an n_row x n_col matrix of NA: (rows, cols, values)"""
    rows = np.repeat(np.arange(n_row, dtype=np.int32), n_col)
    cols = np.tile(np.arange(n_col, dtype=np.int32), n_row)
    vals = np.full(n_row * n_col, NA_LOGICAL, dtype=np.int32) if logical else np.full(n_row * n_col, NA_REAL)
    return rows, cols, vals


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
    """`x[i, j]` for RsparseMatrix — R/slice.R:293-585 (integer / logical / name / negative / sparseVector indices,
    NA entries included: an NA row or column of the result is NA throughout, through inject_NAs).  `drop` and the
    scalar (i, j) lookup (:302-381, extract_single_val_csr_*) are taken under options["mxgpu.slice_drop_route"]
    only.  Branch selection is the reference's (:439-565):
      contiguous ascending rows, all columns      -> host slicing, as the reference does in pure R (:477-483)
      descending rows, all columns                -> host slicing + reverse_rows_*                    (:484-501)
      other rows, all columns                     -> copy_csr_rows_*            (row-gather kernel)   (:502-515)
      contiguous ascending columns                -> copy_csr_rows_col_seq_*                          (:516-529)
      contiguous descending columns               -> copy_csr_rows_col_seq_* + reverse_columns_inplace_* (:530-546)
      anything else                               -> copy_csr_arbitrary_*                             (:547-565)
      full reversal of both                       -> reverse_rows_* + reverse_columns_inplace_*       (:439-469)"""
    check_valid_matrix(x)
    if isinstance(x, StructuredMatrix):
        if x.layout != "R":
            stop("subset_csr takes the row-compressed classes; convert a CsparseMatrix with as_csr_matrix first.")
        if _drop_route() and i is not None and j is not None and _is_scalar_number(i) and _is_scalar_number(j):
            return _subset_csr_single(x, i, j, drop)                # :316-333 come before the lookup
        return subset_csr(structured.as_general(x), i, j, drop)    # :473-474
    if i is None and j is None:
        return drop_slice(x, drop)
    if _drop_route() and i is not None and j is not None and _is_scalar_number(i) and _is_scalar_number(j):
        return _subset_csr_single(x, i, j, drop)
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
        return drop_slice(out, drop)
    if all_i and all_j:                                         # R/slice.R:423-425
        return drop_slice(x, drop)
    kind = _cls_kind(x)
    if P.i_all_NA or P.j_all_NA:
        # R/slice.R:428-437 takes this branch when each axis is all NA or all of it.  An axis that is all NA beside a
        # partial one is NA throughout just the same; the reference goes on with NA_integer_ indices there.
        rows, cols, vals = _na_matrix_entries(n_row, n_col, kind != "d")
        indptr = (np.arange(n_row + 1, dtype=np.int64) * n_col).astype(np.int32)
        names = [_names_without(new_rn, P.i_NAs), _names_without(new_cn, P.j_NAs)]
        return drop_slice((dgRMatrix if kind == "d" else lgRMatrix)(indptr, cols, vals, (n_row, n_col), names), drop)

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
        return drop_slice(res, drop, P.i_NAs, P.j_NAs)          # R/slice.R:583

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


def _subset_csr_single(x, i, j, drop):
    """R/slice.R:302-381, under the drop route: `x[i, j]` with two scalar numbers through extract_single_val_csr_*.
    A scalar (float; TRUE / FALSE / NA_LOGICAL for an lgRMatrix), or with drop=False the 1 x 1 matrix that is empty
    when the value is 0.  A symmetric / triangular operand takes the branches of :316-333 first (0 outside a
    triangular's triangle, 1 on a unit diagonal, (i, j) swapped into a symmetric's stored triangle).  A scalar <= 0
    is no exclusion on this route: it selects nothing and gives 0, as on the COO route (the reference reads row
    i - 1 < 0 of the index pointer there)."""
    i, j = _scalar_index(i), _scalar_index(j)
    nrow, ncol = x.Dim
    known = None
    if isinstance(x, StructuredMatrix):
        if i != NA_INTEGER and j != NA_INTEGER and 1 <= i <= nrow and 1 <= j <= ncol:
            route = structured.scalar_route(x, i, j)
            if route[0] == "value":
                known = route[1]
            else:
                i, j = route[1], route[2]
        x = structured.stored_as_general(x)
    kind = _cls_kind(x)
    if i == NA_INTEGER or j == NA_INTEGER:                      # :309-310
        res = NA_REAL
    elif i > nrow or j > ncol:
        stop("Subscript out of bounds.")
    elif i < 1 or j < 1:
        res = 0.0
    elif known is not None:                                     # :316-322: `res <- 0` / `res <- 1.`, numbers in every kind
        res = known
    elif kind == "d":
        res = exports.extract_single_val_csr_numeric(x.p, x.j, x.x, i - 1, j - 1)
    elif kind == "l":                                           # as.logical() of the int the export returns
        v = exports.extract_single_val_csr_logical(x.p, x.j, x.x, i - 1, j - 1)
        res = NA_LOGICAL if v == NA_LOGICAL else bool(v)
    else:
        res = exports.extract_single_val_csr_binary(x.p, x.j, i - 1, j - 1)
    if drop:
        return res                              # names(res) <- colnames(x)[j] (:347-348) is not mirrored
    is_na = (isinstance(res, float) and np.isnan(res)) or (not isinstance(res, (bool, float)) and res == NA_LOGICAL)
    rn = x.Dimnames[0][i - 1] if x.Dimnames[0] is not None and len(x.Dimnames[0]) and i >= 1 else None
    cn = x.Dimnames[1][j - 1] if x.Dimnames[1] is not None and len(x.Dimnames[1]) and j >= 1 else None
    cls = {"d": dgRMatrix, "l": lgRMatrix, "n": ngRMatrix}[kind]
    names = [None if rn is None else [rn], None if cn is None else [cn]]
    if not is_na and res == 0:                                  # :367-369
        return cls(np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32), None, (1, 1), names)
    # the reference's `if (res == 0)` stops on an NA (:367); here the one cell holds it
    if kind == "d":
        xv = np.array([res], dtype=np.float64)
    elif kind == "l":
        xv = np.array([NA_LOGICAL if is_na else 1], dtype=np.int32)
    else:
        xv = None
    return cls(np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), xv, (1, 1), names)


def _empty_coo(kind, n_row, n_col, row_names, col_names):
    xv = None if kind == "n" else np.zeros(0, dtype=_COO_CLS[kind].value_dtype)
    return _COO_CLS[kind](np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), xv, (n_row, n_col),
                          [row_names, col_names])


def _subset_coo_single(x, i, j, drop):
    """R/slice_coo.R:10-84.  The symmetric / triangular branches (:22-42) concern symmetric / triangular triplet
    classes, which have no stand-in here; a compressed one reaches subset_coo expanded."""
    i, j = _scalar_index(i), _scalar_index(j)                  # as.integer(): truncates
    nrow, ncol = x.Dim
    if i == NA_INTEGER or j == NA_INTEGER:                      # :17-18
        if drop:
            return NA_REAL
        out = _empty_coo(_coo_kind(x), 1, 1, None, None)        # :75-82: the one cell holds the NA
        out.i, out.j = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        if out.x is not None:
            out.x = np.array([NA_REAL]) if isinstance(x, dgTMatrix) else np.array([NA_LOGICAL], dtype=np.int32)
        return out
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
    """`x[i, j]` for TsparseMatrix — R/slice_coo.R:1-232 (integer / logical / name / negative / sparseVector
    indices, NA entries included, through inject_NAs_inplace_coo_*).  As in subset_csr, `drop` to a vector for
    non-scalar selections is taken under options["mxgpu.slice_drop_route"] only; without it `drop` only matters for
    the scalar (i, j) route.  Routes:
      both i and j scalar numbers                 -> slice_coo_single_*, a scalar, or 1 x 1 with drop=False (:10-84)
      empty i or j, or no entries                 -> empty T-matrix of the same kind                      (:108-125)
      all rows and all columns                    -> x itself                                             (:127-129)
      full reversal of both                       -> slice_coo_arbitrary_* with the rev-seq flags; the reference
                                                     flips (nrow-1) - i, (ncol-1) - j in R (:142-154), which the
                                                     kernel's affine reversed axes reproduce bit for bit
      anything else                               -> slice_coo_arbitrary_*                                (:160-196)
    A symmetric / triangular compressed operand is expanded to the TsparseMatrix of its kind first."""
    check_valid_matrix(x)
    if isinstance(x, StructuredMatrix):
        x = as_coo_matrix(x, binary=x.value_dtype is None, logical=x.value_dtype == np.int32)
    if i is None and j is None:
        return drop_slice(x, drop)
    if i is not None and j is not None and _is_scalar_number(i) and _is_scalar_number(j):
        return _subset_coo_single(x, i, j, drop)
    return _subset_coo_vectors(x, i, j, drop)


def _subset_coo_vectors(x, i, j, drop=False):
    """R/slice_coo.R:87-232: everything but the scalar route."""
    P = get_ij_properties(x, i, j)
    kind = _coo_kind(x)
    if P.n_row == 0 or P.n_col == 0 or x.i.size == 0:                  # :108-125
        return drop_slice(_empty_coo(kind, P.n_row, P.n_col, P.row_names, P.col_names), drop)
    if P.all_i and P.all_j:                                             # :127-129
        return drop_slice(x, drop)
    if P.i_all_NA or P.j_all_NA:                                        # :131-140, and as in subset_csr
        rows, cols, vals = _na_matrix_entries(P.n_row, P.n_col, kind != "d")
        names = [_names_without(P.row_names, P.i_NAs), _names_without(P.col_names, P.j_NAs)]
        return drop_slice((dgTMatrix if kind == "d" else lgTMatrix)(rows, cols, vals, (P.n_row, P.n_col), names), drop)
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
    return drop_slice(res, drop, P.i_NAs, P.j_NAs)                      # :203
