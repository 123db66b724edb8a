"""Python twins of the reference's R/RcppExports.R wrappers for the hot path.

Same names, argument order and return shapes as the R side sees them
(R/RcppExports.R:148-150, 360, 388, 564 …): dense results are numpy arrays in
column-major (Fortran) order, list results are dicts with `indptr`, `indices`,
`values`.  Every function goes through the C-ABI of libmxgpu.so
(include/mxgpu.h) — i.e. through the HIP kernels; nothing here computes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MX_F64, MX_LGL, MX_NONE, MX_OP_ADD, MX_OP_AND, MX_OP_MUL, MX_OP_OR,
                   MX_OP_SUB, MX_OP_XOR, ResultInfo, check, ptr)


def _i32(a):
    a = np.asarray(a)
    if a.dtype != np.int32 or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, dtype=np.int32)
    return a


def _f64(a):
    a = np.asarray(a)
    if a.dtype != np.float64 or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, dtype=np.float64)
    return a


def _dense(M, dtype):
    M = np.asarray(M)
    if M.ndim != 2:
        raise ValueError("dense operand must be a 2-d matrix")
    if M.dtype != dtype or not M.flags.f_contiguous:
        M = np.asfortranarray(M, dtype=dtype)
    return M


# ----------------------------------------------------------------------------- SpMM
def _tcrossprod_csr_dense(X_csr_indptr, X_csr_indices, X_csr_values, Y_colmajor, nthreads, dtype, fn):
    p, j, x = _i32(X_csr_indptr), _i32(X_csr_indices), _f64(X_csr_values)
    Y = _dense(Y_colmajor, dtype)
    m, n, K = p.size - 1, Y.shape[0], Y.shape[1]
    out = np.empty((m, n), dtype=dtype, order="F")
    check(fn(ptr(p), ptr(j), ptr(x), m, ptr(Y), n, K, int(nthreads), ptr(out)))
    return out


def tcrossprod_csr_dense_numeric(X_csr_indptr, X_csr_indices, X_csr_values, Y_colmajor, nthreads=1):
    """R/RcppExports.R:148-150 -> src/matmul.cpp:345-359."""
    return _tcrossprod_csr_dense(X_csr_indptr, X_csr_indices, X_csr_values, Y_colmajor, nthreads, np.float64,
                                 _lib.load().mx_tcrossprod_csr_dense_numeric)


def tcrossprod_csr_dense_float32(X_csr_indptr, X_csr_indices, X_csr_values, Y_colmajor, nthreads=1):
    """src/matmul.cpp:361-375 (Y / result are the float32@Data bits; here numpy float32)."""
    return _tcrossprod_csr_dense(X_csr_indptr, X_csr_indices, X_csr_values, Y_colmajor, nthreads, np.float32,
                                 _lib.load().mx_tcrossprod_csr_dense_float32)


def _dense_times_sparse(X_colmajor, indptr, indices, values, nthreads, dtype, fn, extra=None):
    X = _dense(X_colmajor, dtype)
    p, i, x = _i32(indptr), _i32(indices), _f64(values)
    nrows_X, ncols_X, nout = X.shape[0], X.shape[1], p.size - 1
    out = np.empty((nrows_X, nout), dtype=dtype, order="F")
    args = [ptr(X), nrows_X, ncols_X, ptr(p), ptr(i), ptr(x), nout, int(nthreads)]
    if extra is not None:
        args.append(int(extra))
    args.append(ptr(out))
    check(fn(*args))
    return out


def matmul_dense_csc_numeric(X_colmajor, Y_csc_indptr, Y_csc_indices, Y_csc_values, nthreads=1):
    """src/matmul.cpp:221-235."""
    return _dense_times_sparse(X_colmajor, Y_csc_indptr, Y_csc_indices, Y_csc_values, nthreads, np.float64,
                               _lib.load().mx_matmul_dense_csc_numeric)


def matmul_dense_csc_float32(X_colmajor, Y_csc_indptr, Y_csc_indices, Y_csc_values, nthreads=1):
    """src/matmul.cpp:237-251."""
    return _dense_times_sparse(X_colmajor, Y_csc_indptr, Y_csc_indices, Y_csc_values, nthreads, np.float32,
                               _lib.load().mx_matmul_dense_csc_float32)


def tcrossprod_dense_csr_numeric(X_colmajor, Y_csr_indptr, Y_csr_indices, Y_csr_values, nthreads=1, ncols_Y=0):
    """src/matmul.cpp:283-297."""
    return _dense_times_sparse(X_colmajor, Y_csr_indptr, Y_csr_indices, Y_csr_values, nthreads, np.float64,
                               _lib.load().mx_tcrossprod_dense_csr_numeric, extra=ncols_Y)


def tcrossprod_dense_csr_float32(X_colmajor, Y_csr_indptr, Y_csr_indices, Y_csr_values, nthreads=1, ncols_Y=0):
    """src/matmul.cpp:299-313."""
    return _dense_times_sparse(X_colmajor, Y_csr_indptr, Y_csr_indices, Y_csr_values, nthreads, np.float32,
                               _lib.load().mx_tcrossprod_dense_csr_float32, extra=ncols_Y)


# ----------------------------------------------------------------------------- SpMV
def _dvec(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads, ydt, odt, fn):
    p, j, x = _i32(X_csr_indptr), _i32(X_csr_indices), _f64(X_csr_values)
    y = np.ascontiguousarray(y_dense, dtype=ydt)
    m = p.size - 1
    out = np.empty(m, dtype=odt)
    check(fn(ptr(p), ptr(j), ptr(x), m, ptr(y), y.size, int(nthreads), ptr(out)))
    return out


def matmul_csr_dvec_numeric(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads=1):
    """src/matmul.cpp:421-435."""
    return _dvec(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads, np.float64, np.float64,
                 _lib.load().mx_matmul_csr_dvec_numeric)


def matmul_csr_dvec_integer(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads=1):
    """src/matmul.cpp:437-451."""
    return _dvec(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads, np.int32, np.float64,
                 _lib.load().mx_matmul_csr_dvec_integer)


def matmul_csr_dvec_logical(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads=1):
    """src/matmul.cpp:453-467."""
    return _dvec(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads, np.int32, np.float64,
                 _lib.load().mx_matmul_csr_dvec_logical)


def matmul_csr_dvec_float32(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads=1):
    """src/matmul.cpp:469-483."""
    return _dvec(X_csr_indptr, X_csr_indices, X_csr_values, y_dense, nthreads, np.float32, np.float32,
                 _lib.load().mx_matmul_csr_dvec_float32)


# ----------------------------------------------------------------------------- list results
_VDT = {MX_F64: np.float64, MX_LGL: np.int32, _lib.MX_I32: np.int32}


def _finish(res, info, alias_from=None, empty_values_dtype=np.float64):
    lib = _lib.load()
    vdt = _VDT.get(info.values_dtype)
    if info.alias_structure:
        indptr, indices = alias_from          # the INPUT objects themselves, as the reference returns them
        values = np.empty(info.values_len, dtype=vdt)
        check(lib.mx_result_finish(res, None, None, ptr(values)))
        return dict(indptr=indptr, indices=indices, values=values)
    indptr = np.empty(info.indptr_len, dtype=np.int32)
    indices = np.empty(info.nnz, dtype=np.int32)
    values = np.empty(info.values_len if vdt is not None else 0, dtype=vdt if vdt is not None else empty_values_dtype)
    check(lib.mx_result_finish(res, ptr(indptr), ptr(indices), ptr(values) if values.size else None))
    return dict(indptr=indptr, indices=indices, values=values)


def _begin(fn, *args, finish=_finish, **finish_kw):
    """One *_begin export: fn(*args, &result handle, &info), then `finish` copies the result out and releases the
    handle.  Returns (what `finish` returned, info)."""
    res, info = C.c_void_p(), ResultInfo()
    check(fn(*args, C.byref(res), C.byref(info)))
    return finish(res, info, **finish_kw), info


def _same(a, b):
    return a is b


def _elemwise(op, indptr1, indptr2, indices1, indices2, values1, values2, vdt):
    lib = _lib.load()
    # keep object identity visible to the C-ABI as pointer identity (operators.cpp:104-108, :343-346)
    p1 = _i32(indptr1)
    p2 = p1 if _same(indptr1, indptr2) else _i32(indptr2)
    j1 = _i32(indices1)
    j2 = j1 if _same(indices1, indices2) else _i32(indices2)
    v1 = np.ascontiguousarray(values1, dtype=vdt)
    v2 = v1 if _same(values1, values2) else np.ascontiguousarray(values2, dtype=vdt)
    return _begin(lib.mx_csr_elemwise_begin, op, p1.size - 1, ptr(p1), ptr(p2), ptr(j1), ptr(j2), ptr(v1), ptr(v2),
                  j1.size, j2.size, alias_from=(indptr1, indices1))[0]


def multiply_csr_elemwise(indptr1, indptr2, indices1, indices2, values1, values2):
    """R/RcppExports.R:360 -> src/operators.cpp:209-222."""
    return _elemwise(MX_OP_MUL, indptr1, indptr2, indices1, indices2, values1, values2, np.float64)


def logicaland_csr_elemwise(indptr1, indptr2, indices1, indices2, values1, values2):
    """src/operators.cpp:224-237."""
    return _elemwise(MX_OP_AND, indptr1, indptr2, indices1, indices2, values1, values2, np.int32)


def add_csr_elemwise(indptr1, indptr2, indices1, indices2, values1, values2, substract):
    """R/RcppExports.R:388 -> src/operators.cpp:539-554."""
    return _elemwise(MX_OP_SUB if substract else MX_OP_ADD, indptr1, indptr2, indices1, indices2,
                     values1, values2, np.float64)


def logicalor_csr_elemwise(indptr1, indptr2, indices1, indices2, values1, values2, xor_op):
    """src/operators.cpp:556-571."""
    return _elemwise(MX_OP_XOR if xor_op else MX_OP_OR, indptr1, indptr2, indices1, indices2,
                     values1, values2, np.int32)


def _copy_rows(indptr, indices, values, rows_take, value_dtype, vdt):
    lib = _lib.load()
    p, j, rows = _i32(indptr), _i32(indices), _i32(rows_take)
    v = None if values is None else np.ascontiguousarray(values, dtype=vdt)
    return _begin(lib.mx_copy_csr_rows_begin, ptr(p), p.size - 1, ptr(j), ptr(v), value_dtype,
                  0 if v is None else v.size, ptr(rows), rows.size,
                  empty_values_dtype=vdt if vdt is not None else np.float64)[0]


def copy_csr_rows_numeric(indptr, indices, values, rows_take):
    """R/RcppExports.R:564 -> src/slice.cpp:276-291."""
    return _copy_rows(indptr, indices, values, rows_take, MX_F64, np.float64)


def copy_csr_rows_logical(indptr, indices, values, rows_take):
    """src/slice.cpp:293-308."""
    return _copy_rows(indptr, indices, values, rows_take, MX_LGL, np.int32)


def copy_csr_rows_binary(indptr, indices, rows_take):
    """src/slice.cpp:310-324."""
    return _copy_rows(indptr, indices, None, rows_take, MX_NONE, None)


# ----------------------------------------------------------------------------- column-filtering slices (§8f-2)
def _col_seq(indptr, indices, values, rows_take, cols_take, index1, value_dtype, vdt):
    lib = _lib.load()
    p, j, rows, cols = _i32(indptr), _i32(indices), _i32(rows_take), _i32(cols_take)
    v = None if values is None else np.ascontiguousarray(values, dtype=vdt)
    # values are always a numeric (float64) vector, slice.cpp:363
    return _begin(lib.mx_copy_csr_rows_col_seq_begin, ptr(p), p.size - 1, ptr(j), ptr(v), value_dtype,
                  0 if v is None else v.size, ptr(rows), rows.size, ptr(cols), cols.size, int(bool(index1)))[0]


def copy_csr_rows_col_seq_numeric(indptr, indices, values, rows_take, cols_take, index1):
    """R/RcppExports.R:576 -> src/slice.cpp:385-403."""
    return _col_seq(indptr, indices, values, rows_take, cols_take, index1, MX_F64, np.float64)


def copy_csr_rows_col_seq_logical(indptr, indices, values, rows_take, cols_take, index1):
    """src/slice.cpp:405-423 (values come back as numeric, like the reference's NumericVector)."""
    return _col_seq(indptr, indices, values, rows_take, cols_take, index1, MX_LGL, np.int32)


def copy_csr_rows_col_seq_binary(indptr, indices, rows_take, cols_take, index1):
    """src/slice.cpp:425-443."""
    return _col_seq(indptr, indices, None, rows_take, cols_take, index1, MX_NONE, None)


def _arbitrary(indptr, indices, values, rows_take, cols_take, value_dtype, vdt):
    lib = _lib.load()
    p, j, rows, cols = _i32(indptr), _i32(indices), _i32(rows_take), _i32(cols_take)
    v = None if values is None else np.ascontiguousarray(values, dtype=vdt)
    out, info = _begin(lib.mx_copy_csr_arbitrary_begin, ptr(p), p.size - 1, ptr(j), ptr(v), value_dtype,
                       0 if v is None else v.size, ptr(rows), rows.size, ptr(cols), cols.size,
                       empty_values_dtype=vdt if vdt is not None else np.float64)
    if info.values_dtype == MX_NONE:
        del out["values"]              # the reference's list has no `values` element then (slice.cpp:565)
    return out


def copy_csr_arbitrary_numeric(indptr, indices, values, rows_take, cols_take):
    """src/slice.cpp:580-596."""
    return _arbitrary(indptr, indices, values, rows_take, cols_take, MX_F64, np.float64)


def copy_csr_arbitrary_logical(indptr, indices, values, rows_take, cols_take):
    """src/slice.cpp:598-614."""
    return _arbitrary(indptr, indices, values, rows_take, cols_take, MX_LGL, np.int32)


def copy_csr_arbitrary_binary(indptr, indices, rows_take, cols_take):
    """src/slice.cpp:616-632."""
    return _arbitrary(indptr, indices, None, rows_take, cols_take, MX_NONE, None)


def _reverse_rows(indptr, indices, values, value_dtype, vdt):
    lib = _lib.load()
    p, j = _i32(indptr), _i32(indices)
    v = None if values is None else np.ascontiguousarray(values, dtype=vdt)
    return _begin(lib.mx_reverse_rows_begin, ptr(p), p.size - 1, ptr(j), ptr(v), value_dtype,
                  0 if v is None else v.size, empty_values_dtype=vdt if vdt is not None else np.float64)[0]


def reverse_rows_numeric(indptr, indices, values):
    """src/slice.cpp:98-110."""
    return _reverse_rows(indptr, indices, values, MX_F64, np.float64)


def reverse_rows_logical(indptr, indices, values):
    """src/slice.cpp:112-124."""
    return _reverse_rows(indptr, indices, values, MX_LGL, np.int32)


def reverse_rows_binary(indptr, indices):
    """src/slice.cpp:126-138."""
    return _reverse_rows(indptr, indices, None, MX_NONE, None)


def _reverse_columns_inplace(indptr, indices, values, ncol, value_dtype):
    p = _i32(indptr)
    if not (isinstance(indices, np.ndarray) and indices.dtype == np.int32 and indices.flags.c_contiguous):
        raise TypeError("indices must be a contiguous int32 numpy array (modified in place)")
    check(_lib.load().mx_reverse_columns_inplace(ptr(p), p.size - 1, ptr(indices), ptr(values), value_dtype,
                                                 0 if values is None else values.size, int(ncol)))


def reverse_columns_inplace_numeric(indptr, indices, values, ncol):
    """src/slice.cpp:172-187: modifies `indices` / `values`."""
    _reverse_columns_inplace(indptr, indices, values, ncol, MX_F64)


def reverse_columns_inplace_logical(indptr, indices, values, ncol):
    """src/slice.cpp:189-204."""
    _reverse_columns_inplace(indptr, indices, values, ncol, MX_LGL)


def reverse_columns_inplace_binary(indptr, indices, ncol):
    """src/slice.cpp:206-221."""
    _reverse_columns_inplace(indptr, indices, None, ncol, MX_NONE)


# ----------------------------------------------------------------------------- CSR x sparse vector, CSR (.) dense (§8f-4)
def _svec(kind, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads):
    p, j, x, yi = _i32(X_csr_indptr), _i32(X_csr_indices), _f64(X_csr_values), _i32(y_indices_base1)
    yv = None
    if kind == 0:
        yv = _f64(y_values)
    elif kind in (1, 2):
        yv = _i32(y_values)
    elif kind == 4:
        yv = np.ascontiguousarray(y_values, dtype=np.float32)
    out = np.empty(p.size - 1, dtype=np.float64)
    check(_lib.load().mx_matmul_csr_svec(ptr(p), ptr(j), ptr(x), p.size - 1, ptr(yi), yi.size, ptr(yv), kind,
                                         int(nthreads), ptr(out)))
    return out


def matmul_csr_svec_numeric(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads=1):
    """src/matmul.cpp:555-571."""
    return _svec(0, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads)


def matmul_csr_svec_integer(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads=1):
    """src/matmul.cpp:573-589."""
    return _svec(1, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads)


def matmul_csr_svec_logical(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads=1):
    """src/matmul.cpp:591-607."""
    return _svec(2, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads)


def matmul_csr_svec_binary(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, nthreads=1):
    """src/matmul.cpp:609-624."""
    return _svec(3, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, None, nthreads)


def matmul_csr_svec_float32(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads=1):
    """src/matmul.cpp:626-641."""
    return _svec(4, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, nthreads)


# ----------------------------------------------------------------------------- outer products, row vector x CSC (outer.hip)
def _as_f32(a):
    """float32 values; an int32 array is the float32@Data bits, as the R side passes them"""
    a = np.asarray(a)
    if a.dtype == np.int32:
        a = a.view(np.float32)
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _rowvec(rowvec_, indptr, indices, values):
    v, p, i = _as_f32(rowvec_), _i32(indptr), _i32(indices)
    x = None if values is None else _f64(values)
    if i.size < p[-1] or (x is not None and x.size < p[-1]):
        raise ValueError("indices / values shorter than the index pointer says")
    out = np.empty((1, p.size - 1), dtype=np.float32, order="F")
    check(_lib.load().mx_matmul_rowvec_by_csc(ptr(v), v.size, ptr(p), p.size - 1, ptr(i), ptr(x), ptr(out)))
    return out


def matmul_rowvec_by_csc(rowvec_, indptr, indices, values):
    """src/matmul.cpp:643-663: a 1 x ncol float32 matrix (the reference's IntegerMatrix of float bits)."""
    return _rowvec(rowvec_, indptr, indices, values)


def matmul_rowvec_by_cscbin(rowvec_, indptr, indices):
    """src/matmul.cpp:665-684."""
    return _rowvec(rowvec_, indptr, indices, None)


def _outer_dense(colvec, dtype, indptr, indices, values_):
    p, j, x = _i32(indptr), _i32(indices), _f64(values_)
    if x.size < p[-1]:
        raise ValueError("values shorter than the index pointer says")
    return _begin(_lib.load().mx_matmul_colvec_by_scolvecascsr_begin, ptr(colvec), dtype, colvec.size, ptr(p),
                  p.size - 1, ptr(j), ptr(x))[0]


def matmul_colvec_by_scolvecascsr_f32(colvec_, indptr, indices, values_):
    """src/matmul.cpp:747-762.  The arrays have out_indptr[-1] entries; the reference pads them with zeros to
    length(indices) * length(colvec) when a row stores more than one entry."""
    return _outer_dense(_as_f32(colvec_), _lib.MX_F32, indptr, indices, values_)


def matmul_colvec_by_scolvecascsr(colvec_, indptr, indices, values_):
    """src/matmul.cpp:766-781."""
    return _outer_dense(_f64(colvec_).reshape(-1), MX_F64, indptr, indices, values_)


def _outer_svec(value_dtype, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, y_length):
    p, j, x, yi = _i32(X_csr_indptr), _i32(X_csr_indices), _f64(X_csr_values), _i32(y_indices_base1)
    yv = None
    if value_dtype == MX_F64:
        yv = _f64(y_values)
    elif value_dtype != MX_NONE:
        yv = _i32(y_values)
    if x.size < p[-1] or (yv is not None and yv.size != yi.size):
        raise ValueError("values and index vectors have different lengths")
    return _begin(_lib.load().mx_matmul_spcolvec_by_scolvecascsr_begin, ptr(p), p.size - 1, ptr(j), ptr(x), ptr(yi),
                  ptr(yv), value_dtype, yi.size, int(y_length))[0]


def matmul_spcolvec_by_scolvecascsr_numeric(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values,
                                            y_length):
    """src/matmul.cpp:857-876 (with y_values[k] where :808 reads y_values[col])."""
    return _outer_svec(MX_F64, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, y_length)


def matmul_spcolvec_by_scolvecascsr_integer(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values,
                                            y_length):
    """src/matmul.cpp:878-897."""
    return _outer_svec(_lib.MX_I32, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, y_length)


def matmul_spcolvec_by_scolvecascsr_logical(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values,
                                            y_length):
    """src/matmul.cpp:899-918."""
    return _outer_svec(MX_LGL, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_values, y_length)


def matmul_spcolvec_by_scolvecascsr_binary(X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, y_length):
    """src/matmul.cpp:920-938."""
    return _outer_svec(MX_NONE, X_csr_indptr, X_csr_indices, X_csr_values, y_indices_base1, None, y_length)


def _csr_by_dense(kind, indptr, indices, values, dense_mat):
    p, j = _i32(indptr), _i32(indices)
    ddt = {0: np.float64, 1: np.float32, 2: np.int32, 3: np.int32, 4: np.int32}[kind]
    D = _dense(dense_mat, ddt)
    if D.shape[0] != p.size - 1:
        raise ValueError("dense operand must have as many rows as the sparse one")
    xv = np.ascontiguousarray(values, dtype=np.int32 if kind == 4 else np.float64)
    out = np.empty(xv.size, dtype=xv.dtype)
    check(_lib.load().mx_multiply_csr_by_dense_elemwise(ptr(p), ptr(j), ptr(xv), p.size - 1, ptr(D), D.shape[1], kind,
                                                        ptr(out)))
    return out


def multiply_csr_by_dense_elemwise_double(indptr, indices, values, dense_mat):
    """src/operators.cpp:289-296."""
    return _csr_by_dense(0, indptr, indices, values, dense_mat)


def multiply_csr_by_dense_elemwise_float32(indptr, indices, values, dense_mat):
    """src/operators.cpp:298-305."""
    return _csr_by_dense(1, indptr, indices, values, dense_mat)


def multiply_csr_by_dense_elemwise_int(indptr, indices, values, dense_mat):
    """src/operators.cpp:307-314."""
    return _csr_by_dense(2, indptr, indices, values, dense_mat)


def multiply_csr_by_dense_elemwise_bool(indptr, indices, values, dense_mat):
    """src/operators.cpp:316-323."""
    return _csr_by_dense(3, indptr, indices, values, dense_mat)


def logicaland_csr_by_dense_cpp(indptr, indices, values, dense_mat):
    """src/operators.cpp:325-334."""
    return _csr_by_dense(4, indptr, indices, values, dense_mat)


# ----------------------------------------------------------------------------- CSC (.) dense (svec.hip, cscdense.hip)
_CSC_DENSE_DT = {0: np.float64, 1: np.float32, 2: np.int32, 3: np.int32, 4: np.int32}


def _csc_dense_args(kind, indptr, indices, values, dense_):
    p, i = _i32(indptr), _i32(indices)
    D = _dense(dense_, _CSC_DENSE_DT[kind])
    if p.size < 1 or D.shape[1] != p.size - 1:
        raise ValueError("dense operand must have as many columns as the sparse one")
    xv = np.ascontiguousarray(values, dtype=np.int32 if kind == 4 else np.float64)
    if xv.size != i.size:
        raise ValueError("indices and values have different lengths")
    return p, i, xv, D


def _csc_by_dense_ignore(fn, kind, indptr, indices, values, dense_):
    p, i, xv, D = _csc_dense_args(kind, indptr, indices, values, dense_)
    out = np.empty(xv.size, dtype=xv.dtype)
    check(fn(ptr(p), p.size - 1, ptr(i), ptr(xv), ptr(D), D.shape[0], ptr(out)))
    return out


def _csc_by_dense_keep(fn, kind, indptr, indices, values, dense_):
    p, i, xv, D = _csc_dense_args(kind, indptr, indices, values, dense_)
    return _begin(fn, ptr(p), p.size - 1, ptr(i), ptr(xv), ptr(D), D.shape[0])[0]


def multiply_csc_by_dense_ignore_NAs_numeric(indptr, indices, values, dense_):
    """src/operators.cpp:1125-1139: x * d for every entry of the CSC, in storage order (values only)."""
    return _csc_by_dense_ignore(_lib.load().mx_multiply_csc_by_dense_ignore_NAs_numeric, 0, indptr, indices, values,
                                dense_)


def multiply_csc_by_dense_ignore_NAs_float32(indptr, indices, values, dense_):
    """src/operators.cpp:1140-1155: dense_ holds the float32 values (float32@Data), widened to f64 per entry."""
    return _csc_by_dense_ignore(_lib.load().mx_multiply_csc_by_dense_ignore_NAs_float32, 1, indptr, indices, values,
                                dense_)


def multiply_csc_by_dense_ignore_NAs_integer(indptr, indices, values, dense_):
    """src/operators.cpp:1157-1172: an NA_INTEGER cell gives NA_real_."""
    return _csc_by_dense_ignore(_lib.load().mx_multiply_csc_by_dense_ignore_NAs_integer, 2, indptr, indices, values,
                                dense_)


def multiply_csc_by_dense_ignore_NAs_logical(indptr, indices, values, dense_):
    """src/operators.cpp:1174-1189: R logical dense (int32 or bool); NA gives NA_real_."""
    return _csc_by_dense_ignore(_lib.load().mx_multiply_csc_by_dense_ignore_NAs_logical, 3, indptr, indices, values,
                                dense_)


def logicaland_csc_by_dense_ignore_NAs(indptr, indices, values, dense_):
    """src/operators.cpp:1191-1206: R logicals in and out, R's three-valued AND."""
    return _csc_by_dense_ignore(_lib.load().mx_logicaland_csc_by_dense_ignore_NAs, 4, indptr, indices, values, dense_)


def multiply_csc_by_dense_keep_NAs_numeric(indptr, indices_, values, dense_):
    """src/operators.cpp:1388-1404: dict(indptr, indices, values) of the product with the NA cells of dense_ that lie
    outside the pattern added as NA_real_ entries.  Rows must be sorted inside each column; a repeated row is kept
    once, with the first entry's value."""
    return _csc_by_dense_keep(_lib.load().mx_multiply_csc_by_dense_keep_NAs_numeric, 0, indptr, indices_, values,
                              dense_)


def multiply_csc_by_dense_keep_NAs_integer(indptr, indices_, values, dense_):
    """src/operators.cpp:1406-1422 (NA cells: NA_INTEGER)."""
    return _csc_by_dense_keep(_lib.load().mx_multiply_csc_by_dense_keep_NAs_integer, 2, indptr, indices_, values,
                              dense_)


def multiply_csc_by_dense_keep_NAs_logical(indptr, indices_, values, dense_):
    """src/operators.cpp:1424-1440 (NA cells: NA_LOGICAL)."""
    return _csc_by_dense_keep(_lib.load().mx_multiply_csc_by_dense_keep_NAs_logical, 3, indptr, indices_, values,
                              dense_)


def multiply_csc_by_dense_keep_NAs_float32(indptr, indices_, values, dense_):
    """src/operators.cpp:1442-1458 (NA cells: any float32 NaN)."""
    return _csc_by_dense_keep(_lib.load().mx_multiply_csc_by_dense_keep_NAs_float32, 1, indptr, indices_, values,
                              dense_)


# ----------------------------------------------------------------------------- cbind / rbind (§8f-3)
def _cbind(Xp, Xj, Xx, Yp, Yj_plus_ncol, Yx, value_dtype, vdt):
    lib = _lib.load()
    Xp, Xj, Yp, Yj = _i32(Xp), _i32(Xj), _i32(Yp), _i32(Yj_plus_ncol)
    xv = None if Xx is None else np.ascontiguousarray(Xx, dtype=vdt)
    yv = None if Yx is None else np.ascontiguousarray(Yx, dtype=vdt)
    return _begin(lib.mx_cbind_csr_begin, ptr(Xp), Xp.size - 1, ptr(Xj), ptr(xv), 0 if xv is None else xv.size,
                  ptr(Yp), Yp.size - 1, ptr(Yj), ptr(yv), 0 if yv is None else yv.size, value_dtype)[0]


def cbind_csr_numeric(X_csr_indptr, X_csr_indices, X_csr_values, Y_csr_indptr, Y_csr_indices_plus_ncol, Y_csr_values):
    """src/cbind.cpp:101-119."""
    return _cbind(X_csr_indptr, X_csr_indices, X_csr_values, Y_csr_indptr, Y_csr_indices_plus_ncol, Y_csr_values,
                  MX_F64, np.float64)


def cbind_csr_logical(X_csr_indptr, X_csr_indices, X_csr_values, Y_csr_indptr, Y_csr_indices_plus_ncol, Y_csr_values):
    """src/cbind.cpp:121-139."""
    return _cbind(X_csr_indptr, X_csr_indices, X_csr_values, Y_csr_indptr, Y_csr_indices_plus_ncol, Y_csr_values,
                  MX_LGL, np.int32)


def cbind_csr_binary(X_csr_indptr, X_csr_indices, Y_csr_indptr, Y_csr_indices_plus_ncol):
    """src/cbind.cpp:141-157."""
    return _cbind(X_csr_indptr, X_csr_indices, None, Y_csr_indptr, Y_csr_indices_plus_ncol, None, MX_NONE, None)


_RbindInput = _lib.RbindInput      # mx_rbind_input, as include/mxgpu.h declares it


def concat_csr_batch(objects, out_kind):
    """concat_csr_batch (src/rbind.cpp:24-173) over plain arrays: objects = list of
    (kind, indptr|None, indices, values|None, nrows) with kind 0 dgR, 1 lgR, 2 ngR, 3/4/5/6 d/i/l/n sparseVector
    (1-based indices, one row); out_kind 0 dgR, 1 lgR, 2 ngR.  Returns dict(indptr, indices, values)."""
    lib = _lib.load()
    keep, arr = [], (_RbindInput * max(len(objects), 1))()
    for k, (kind, p, j, x, nr) in enumerate(objects):
        jj = _i32(j)
        pp = None if p is None else _i32(p)
        xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64 if kind in (0, 3) else np.int32)
        keep += [jj, pp, xx]
        arr[k] = _RbindInput(kind, None if pp is None else pp.ctypes.data, jj.ctypes.data,
                             None if xx is None else xx.ctypes.data, int(nr), jj.size)
    out = _begin(lib.mx_concat_csr_batch_begin, arr, len(objects), out_kind)[0]
    if out_kind == 2:
        out["values"] = None
    return out


def rbind_coo(objects, out_kind, row_offsets=None):
    """rbind2_coo / rbind2_coo_vec (R/rbind.R:405-520) over plain arrays: objects = list of
    (kind, i|None, j, values|None, nrows) with kind 0 dgT, 1 lgT, 2 ngT (0-based i, j), 3/4/5/6 d/i/l/n sparseVector
    (i None, j = its 1-based indices, one row); out_kind 0 dgT, 1 lgT, 2 ngT; row_offsets = each operand's first
    output row (default: one below the other, in the order given).  Returns dict(ii, jj, xx), xx None for
    out_kind 2: the COO shape slice_coo_arbitrary_* return."""
    lib = _lib.load()
    keep, arr = [], (_RbindInput * max(len(objects), 1))()
    for k, (kind, i, j, x, nr) in enumerate(objects):
        jj = _i32(j)
        ii = None if i is None else _i32(i)
        if ii is not None and ii.size != jj.size:
            raise ValueError("row and column indices have different length")
        xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64 if kind in (0, 3) else np.int32)
        if xx is not None and xx.size != jj.size:
            raise ValueError("indices and values have different number of entries")
        keep += [jj, ii, xx]
        arr[k] = _RbindInput(kind, None if ii is None else ii.ctypes.data, jj.ctypes.data,
                             None if xx is None else xx.ctypes.data, int(nr), jj.size)
    offs = None if row_offsets is None else _i32(row_offsets)
    if offs is not None and offs.size != len(objects):
        raise ValueError("one row offset per operand")
    out = _begin(lib.mx_rbind_coo_begin, arr, len(objects), ptr(offs), out_kind)[0]
    return dict(ii=out["indptr"], jj=out["indices"], xx=None if out_kind == 2 else out["values"])


def cbind_csr_svec(X_csr_indptr, X_csr_indices, X_csr_values, ncols_X, x_kind, v_indices_base1, v_values, v_kind,
                   length, first, out_kind):
    """cbind2(RsparseMatrix, sparseVector) (first=False) / cbind2(sparseVector, RsparseMatrix) (first=True): X of
    x_kind 0 dgR, 1 lgR, 2 ngR with the vector (v_kind 3/4/5/6 d/i/l/n sparseVector, 1-based indices in any order)
    as one more column.  Returns dict(indptr, indices, values), values None for out_kind 2."""
    p, j, vi = _i32(X_csr_indptr), _i32(X_csr_indices), _i32(v_indices_base1)
    xv = None if x_kind == 2 else np.ascontiguousarray(X_csr_values, dtype=np.float64 if x_kind == 0 else np.int32)
    vv = None if v_kind == 6 else np.ascontiguousarray(v_values, dtype=np.float64 if v_kind == 3 else np.int32)
    if (xv is not None and xv.size != j.size) or (vv is not None and vv.size != vi.size):
        raise ValueError("indices and values have different number of entries")
    out = _begin(_lib.load().mx_cbind_csr_svec_begin, ptr(p), p.size - 1, int(ncols_X), ptr(j), ptr(xv), x_kind,
                 ptr(vi), ptr(vv), v_kind, vi.size, int(length), int(bool(first)), out_kind)[0]
    if out_kind == 2:
        out["values"] = None
    return out


def dense_to_svec(dense, dtype):
    """A dense numeric (MX_F64) / integer (MX_I32) / logical (MX_LGL) vector as the (1-based positions, f64 values) of
    a dsparseVector: cells that are zero are dropped, NA / NaN cells stay (NA_integer_ / NA -> NA_real_, TRUE -> 1).
    Returns dict(ii, xx)."""
    a = np.ascontiguousarray(dense, dtype=np.float64 if dtype == MX_F64 else np.int32).reshape(-1)
    out = _begin(_lib.load().mx_dense_to_svec_begin, ptr(a), a.size, dtype)[0]
    return dict(ii=out["indices"], xx=out["values"])


def check_is_seq(indices) -> bool:
    """src/slice.cpp:25-35."""
    a = _i32(indices)
    r = C.c_int(0)
    check(_lib.load().mx_check_is_seq(ptr(a), a.size, C.byref(r)))
    return bool(r.value)


def check_is_rev_seq(indices) -> bool:
    """src/slice.cpp:37-47."""
    a = _i32(indices)
    r = C.c_int(0)
    check(_lib.load().mx_check_is_rev_seq(ptr(a), a.size, C.byref(r)))
    return bool(r.value)


# ----------------------------------------------------------------------------- sort precondition (§8f-1)
def check_indices_are_sorted(indptr, indices) -> bool:
    """Per-row check_is_sorted, src/misc.cpp:118-128."""
    p, j = _i32(indptr), _i32(indices)
    r = C.c_int(0)
    check(_lib.load().mx_check_indices_are_sorted(ptr(p), ptr(j), p.size - 1, C.byref(r)))
    return bool(r.value)


def sort_sparse_indices_inplace(indptr, indices, values=None):
    """sort_sparse_indices_{numeric,logical}_known_ncol / _binary (src/misc.cpp:333-378): sorts the given
    int32 `indices` (and `values`) arrays IN PLACE, like the R-side call does."""
    p = _i32(indptr)
    if not (isinstance(indices, np.ndarray) and indices.dtype == np.int32 and indices.flags.c_contiguous):
        raise TypeError("indices must be a contiguous int32 numpy array (sorted in place)")
    if values is None:
        vd = MX_NONE
    elif values.dtype == np.float64:
        vd = MX_F64
    elif values.dtype == np.int32:
        vd = MX_LGL
    else:
        raise TypeError("values must be float64 or int32 (R logical)")
    check(_lib.load().mx_sort_sparse_indices(ptr(p), ptr(indices), ptr(values), vd, p.size - 1))


def _sort_vector(ii, xx, vd, vdt):
    if not (isinstance(ii, np.ndarray) and ii.dtype == np.int32 and ii.flags.c_contiguous):
        raise TypeError("ii must be a contiguous int32 numpy array (sorted in place)")
    if vdt is not None:
        if not (isinstance(xx, np.ndarray) and xx.dtype == vdt and xx.flags.c_contiguous):
            raise TypeError(f"xx must be a contiguous {np.dtype(vdt).name} numpy array (sorted in place)")
        if xx.size != ii.size:
            raise ValueError("ii and xx have different lengths")
    check(_lib.load().mx_sort_vector_indices(ptr(ii), None if vdt is None else ptr(xx), ii.size, vd))


def sort_vector_indices_numeric(ii, xx):
    """src/misc.cpp:489-497: sorts a sparse vector's `ii` and f64 `xx` IN PLACE by ii; left alone when sorted."""
    _sort_vector(ii, xx, MX_F64, np.float64)


def sort_vector_indices_integer(ii, xx):
    """src/misc.cpp:499-507."""
    _sort_vector(ii, xx, _lib.MX_I32, np.int32)


def sort_vector_indices_logical(ii, xx):
    """src/misc.cpp:509-517."""
    _sort_vector(ii, xx, MX_LGL, np.int32)


def sort_vector_indices_binary(ii):
    """src/misc.cpp:519-527."""
    _sort_vector(ii, None, MX_NONE, None)


def _sort_coo(ii, jj, xx, vd, vdt):
    for name, a in (("indices1", ii), ("indices2", jj)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous):
            raise TypeError(f"{name} must be a contiguous int32 numpy array (sorted in place)")
    if jj.size != ii.size:
        raise ValueError("indices1 and indices2 have different lengths")
    if vdt is not None:
        if not (isinstance(xx, np.ndarray) and xx.dtype == vdt and xx.flags.c_contiguous):
            raise TypeError(f"values must be a contiguous {np.dtype(vdt).name} numpy array (sorted in place)")
        if xx.size != ii.size:
            raise ValueError("indices1 and values have different lengths")
    check(_lib.load().mx_sort_coo_indices(ptr(ii), ptr(jj), None if vdt is None else ptr(xx), ii.size, vd))


def sort_coo_indices_numeric(indices1, indices2, values):
    """src/misc.cpp:430-438: sorts a TsparseMatrix's triplets IN PLACE by (indices1, indices2), stably (entries of
    one cell keep their input order); left alone when sorted."""
    _sort_coo(indices1, indices2, values, MX_F64, np.float64)


def sort_coo_indices_logical(indices1, indices2, values):
    """src/misc.cpp:440-448."""
    _sort_coo(indices1, indices2, values, MX_LGL, np.int32)


def sort_coo_indices_binary(indices1, indices2):
    """src/misc.cpp:450-457."""
    _sort_coo(indices1, indices2, None, MX_NONE, None)


def _csr_by_svec(indptr, indices, values, ii_base1, xx, ncols, length, keep_NAs):
    p, j, x, vi = _i32(indptr), _i32(indices), _f64(values), _i32(ii_base1)
    vx = None if xx is None or (np.asarray(xx).size == 0 and vi.size != 0) else _f64(xx)
    if x.size != j.size:
        raise ValueError("indices and values have different lengths")
    if vx is not None and vx.size != vi.size:
        raise ValueError("ii and xx have different lengths")
    return _begin(_lib.load().mx_multiply_csr_by_svec_begin, ptr(p), p.size - 1, ptr(j), ptr(x), ptr(vi), ptr(vx),
                  vi.size, int(ncols), int(length), int(bool(keep_NAs)))[0]


def multiply_csr_by_svec_no_NAs(indptr, indices, values, ii_base1, xx, length):
    """src/operators.cpp:3426-3498: the rows that the sorted sparse vector stores (recycled every `length` rows),
    scaled by its values; an empty `xx` with a non-empty `ii_base1` is an nsparseVector (values copied)."""
    return _csr_by_svec(indptr, indices, values, ii_base1, xx, 0, length, False)


def multiply_csr_by_svec_keep_NAs(indptr, indices, values, ii_base1, xx, ncols, length):
    """src/operators.cpp:3500-3697: as above, keeping what R's arithmetic makes NA: the NaN / Inf entries of the rows
    the vector does not store, and every column of a row whose vector value is NaN / Inf."""
    return _csr_by_svec(indptr, indices, values, ii_base1, xx, ncols, length, True)


def multiply_csr_by_dvec_no_NAs_numeric(indptr, indices, values, dvec, ncols, multiply, powerto, divide, divrest,
                                        intdiv, X_is_LHS):
    """src/operators.cpp:2142-2175 (R/RcppExports.R:480-482): values-only `X op v` / `v op X` with R's recycling."""
    p, j = _i32(indptr), _i32(indices)
    xv = np.ascontiguousarray(values, dtype=np.float64)
    dv = np.ascontiguousarray(dvec, dtype=np.float64).reshape(-1)
    out = np.empty(xv.size, dtype=np.float64)
    check(_lib.load().mx_multiply_csr_by_dvec_no_NAs_numeric(
        ptr(p), ptr(j), ptr(xv), p.size - 1, ptr(dv), dv.size, int(ncols), bool(multiply), bool(powerto), bool(divide),
        bool(divrest), bool(intdiv), bool(X_is_LHS), ptr(out)))
    return out


def multiply_csr_by_dvec_with_NAs(indptr, indices, values, dvec, ncols, multiply, powerto, divide, divrest, intdiv,
                                  X_is_LHS):
    """src/operators.cpp:2258-2852 (R/RcppExports.R `multiply_csr_by_dvec_with_NAs`): `X op v` with the cells that R
    makes NA / NaN / 1 / Inf outside X's pattern added; rows of X sorted.  When the flat regime adds nothing, `indptr`
    and `indices` of the result are the argument objects themselves, as in the reference (:2643-2651)."""
    p, j, x = _i32(indptr), _i32(indices), _f64(values)
    dv = np.ascontiguousarray(dvec, dtype=np.float64).reshape(-1)
    if x.size != j.size:
        raise ValueError("indices and values have different lengths")
    return _begin(_lib.load().mx_multiply_csr_by_dvec_with_NAs_begin, ptr(p), ptr(j), ptr(x), p.size - 1, ptr(dv),
                  dv.size, int(ncols), bool(multiply), bool(powerto), bool(divide), bool(divrest), bool(intdiv),
                  bool(X_is_LHS), alias_from=(indptr, indices))[0]


def logicaland_csr_by_dvec_internal(indptr, indices, values, dvec, ncols):
    """src/operators.cpp:2177-2200 (R/RcppExports.R:484-486): R logicals in, R logicals out."""
    p, j = _i32(indptr), _i32(indices)
    xv = np.ascontiguousarray(values, dtype=np.int32)
    dv = np.ascontiguousarray(dvec, dtype=np.int32).reshape(-1)
    out = np.empty(xv.size, dtype=np.int32)
    check(_lib.load().mx_logicaland_csr_by_dvec_internal(ptr(p), ptr(j), ptr(xv), p.size - 1, ptr(dv), dv.size,
                                                         int(ncols), ptr(out)))
    return out


# ----------------------------------------------------------------------------- transpose (t_deep, CSR <-> CSC)
def csr_transpose(indptr, indices, values, ncol):
    """CSR arrays of the transpose of an (len(indptr)-1) x ncol CSR; CSC input is the CSR of its transpose, so this
    is also CSR -> CSC and CSC -> CSR.  Replaces t_deep_internal (R/trans.R:46-56) and the Matrix coercions of
    as.csr.matrix / as.csc.matrix (R/conversions.R).  values: float64, int32 R logicals, or None (pattern; the
    result's `values` is then None).  Output rows are in ascending source-row order; repeated (row, col) pairs are
    merged (f64 summed in source order, logicals by R's `|`, pattern once)."""
    lib = _lib.load()
    p, j = _i32(indptr), _i32(indices)
    if values is None:
        v, vdt = None, MX_NONE
    else:
        v = np.asarray(values)
        if v.dtype == np.int32:
            vdt = MX_LGL
        elif v.dtype == np.float64:
            vdt = MX_F64
        else:
            raise TypeError(f"values must be float64 or int32 (R logical), got {v.dtype}")
        v = np.ascontiguousarray(v)
    out = _begin(lib.mx_csr_transpose_begin, ptr(p), p.size - 1, int(ncol), ptr(j), ptr(v), vdt,
                 0 if v is None else v.size, empty_values_dtype=np.float64 if v is None else v.dtype)[0]
    # no entries: an empty vector of the input's type
    out["values"] = None if v is None else out["values"].astype(v.dtype, copy=False)
    return out


# ----------------------------------------------------------------------------- COO (TsparseMatrix)
def _values_kind(values):
    """(array, mx dtype) of a value vector: float64, int32 R logicals, or None (pattern)."""
    if values is None:
        return None, MX_NONE
    v = np.asarray(values)
    if v.dtype == np.int32:
        return np.ascontiguousarray(v), MX_LGL
    if v.dtype == np.float64:
        return np.ascontiguousarray(v), MX_F64
    raise TypeError(f"values must be float64 or int32 (R logical), got {v.dtype}")


def coo_to_csr(i, j, values, nrow, ncol):
    """CSR arrays of an nrow x ncol COO (0-based triplets, any order, duplicates allowed): Matrix's
    TsparseMatrix -> RsparseMatrix coercion behind as.csr.matrix (R/conversions.R:180-295).  Rows come out with
    ascending, unique columns; repeated (i, j) pairs are merged (f64 summed in input order, logicals by R's `|`,
    pattern once).  coo_to_csr(j, i, x, ncol, nrow) gives the CSC arrays.  values None -> `values` is None."""
    lib = _lib.load()
    ri, cj = _i32(i), _i32(j)
    if ri.size != cj.size:
        raise ValueError("row and column indices have different length")
    v, vdt = _values_kind(values)
    if v is not None and v.size != ri.size:
        raise ValueError("values and indices have different number of entries")
    out = _begin(lib.mx_coo_to_csr_begin, ptr(ri), ptr(cj), ptr(v), vdt, ri.size, int(nrow), int(ncol),
                 empty_values_dtype=np.float64 if v is None else v.dtype)[0]
    out["values"] = None if v is None else out["values"].astype(v.dtype, copy=False)
    return out


def csr_to_coo(indptr):
    """Row id of every entry of a CSR (column id, for a CSC), in storage order: the index vector as.coo.matrix
    adds (R/conversions.R:515-590)."""
    p = _i32(indptr)
    out = np.empty(int(p[-1]) if p.size else 0, dtype=np.int32)
    check(_lib.load().mx_csr_to_coo(ptr(p), p.size - 1, ptr(out)))
    return out


def _csr_by_coo(logical, X_csr_indptr, X_csr_indices, X_csr_values, Y_coo_row, Y_coo_col, Y_coo_val, max_row_X,
                max_col_X):
    lib = _lib.load()
    vdt = np.int32 if logical else np.float64
    p, xj = _i32(X_csr_indptr), _i32(X_csr_indices)
    xv = np.ascontiguousarray(X_csr_values, dtype=vdt)
    yi, yj = _i32(Y_coo_row), _i32(Y_coo_col)
    yv = np.ascontiguousarray(Y_coo_val, dtype=vdt)
    if not (yi.size == yj.size == yv.size):
        raise ValueError("COO row, column and value vectors have different lengths")
    if p.size != int(max_row_X) + 1:
        raise ValueError("X_csr_indptr must have max_row_X + 1 entries")
    out = _begin(lib.mx_multiply_csr_by_coo_begin, int(bool(logical)), ptr(p), ptr(xj), ptr(xv), ptr(yi), ptr(yj),
                 ptr(yv), yi.size, int(max_row_X), int(max_col_X), empty_values_dtype=vdt)[0]
    return dict(row=out["indptr"], col=out["indices"], val=out["values"].astype(vdt, copy=False))


def multiply_csr_by_coo_elemwise(X_csr_indptr, X_csr_indices, X_csr_values, Y_coo_row, Y_coo_col, Y_coo_val,
                                 max_row_X, max_col_X):
    """src/operators.cpp:673-696: dict(row, col, val) of the kept COO entries, in Y's input order."""
    return _csr_by_coo(False, X_csr_indptr, X_csr_indices, X_csr_values, Y_coo_row, Y_coo_col, Y_coo_val,
                       max_row_X, max_col_X)


def logicaland_csr_by_coo_elemwise(X_csr_indptr, X_csr_indices, X_csr_values, Y_coo_row, Y_coo_col, Y_coo_val,
                                   max_row_X, max_col_X):
    """src/operators.cpp:698-720: R logicals in and out."""
    return _csr_by_coo(True, X_csr_indptr, X_csr_indices, X_csr_values, Y_coo_row, Y_coo_col, Y_coo_val,
                       max_row_X, max_col_X)


def multiply_coo_by_dense_ignore_NAs_numeric(ii, jj, xx, dvec, nrows, ncols, multiply, powerto, divide, divrest,
                                             intdiv, X_is_LHS):
    """src/operators.cpp:3363-3394: values-only `X op v` / `v op X` of a COO with R's recycling."""
    i, j = _i32(ii), _i32(jj)
    xv = np.ascontiguousarray(xx, dtype=np.float64)
    dv = np.ascontiguousarray(dvec, dtype=np.float64).reshape(-1)
    out = np.empty(xv.size, dtype=np.float64)
    check(_lib.load().mx_multiply_coo_by_dense_ignore_NAs_numeric(
        ptr(i), ptr(j), ptr(xv), xv.size, ptr(dv), dv.size, int(nrows), int(ncols), bool(multiply), bool(powerto),
        bool(divide), bool(divrest), bool(intdiv), bool(X_is_LHS), ptr(out)))
    return out


def multiply_coo_by_dense_ignore_NAs_logical(ii, jj, xx, dvec, nrows, ncols):
    """src/operators.cpp:3396-3418: R logicals in, R logicals out (3-valued AND)."""
    i, j = _i32(ii), _i32(jj)
    xv = np.ascontiguousarray(xx, dtype=np.int32)
    dv = np.ascontiguousarray(dvec, dtype=np.int32).reshape(-1)
    out = np.empty(xv.size, dtype=np.int32)
    check(_lib.load().mx_multiply_coo_by_dense_ignore_NAs_logical(
        ptr(i), ptr(j), ptr(xv), xv.size, ptr(dv), dv.size, int(nrows), int(ncols), ptr(out)))
    return out


# ----------------------------------------------------------------------------- COO slicing (X[i, j] of a TsparseMatrix)
def _slice_coo_arbitrary(ii, jj, xx, vdt, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq, j_is_seq,
                         i_is_rev_seq, j_is_rev_seq, nrows, ncols):
    lib = _lib.load()
    i, j = _i32(ii), _i32(jj)
    if i.size != j.size:
        raise ValueError("row and column indices have different length")
    v = None
    if vdt != MX_NONE:
        v = np.ascontiguousarray(xx, dtype=np.float64 if vdt == MX_F64 else np.int32)
        if v.size != i.size:
            raise ValueError("values and indices have different number of entries")
    rt, ct = _i32(rows_take_base1).reshape(-1), _i32(cols_take_base1).reshape(-1)
    out = _begin(lib.mx_slice_coo_arbitrary_begin, ptr(i), ptr(j), ptr(v), vdt, i.size, ptr(rt), rt.size, ptr(ct),
                 ct.size, bool(all_i), bool(all_j), bool(i_is_seq), bool(j_is_seq), bool(i_is_rev_seq),
                 bool(j_is_rev_seq), int(nrows), int(ncols),
                 empty_values_dtype=np.float64 if v is None else v.dtype)[0]
    xx_out = None if v is None else out["values"].astype(v.dtype, copy=False)
    return dict(ii=out["indptr"], jj=out["indices"], xx=xx_out)


def slice_coo_arbitrary_numeric(ii, jj, xx, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq, j_is_seq,
                                i_is_rev_seq, j_is_rev_seq, nrows, ncols):
    """src/slice_coo.cpp:123-706 (f64): dict(ii, jj, xx) of the selected triplets, 0-based in the result's
    coordinates.  Triplet k gives one output per (position of ii[k]+1 in rows_take_base1, position of jj[k]+1 in
    cols_take_base1), row positions outer, both ascending, triplets in storage order; values copied bit for bit."""
    return _slice_coo_arbitrary(ii, jj, xx, MX_F64, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq,
                                j_is_seq, i_is_rev_seq, j_is_rev_seq, nrows, ncols)


def slice_coo_arbitrary_logical(ii, jj, xx, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq, j_is_seq,
                                i_is_rev_seq, j_is_rev_seq, nrows, ncols):
    """src/slice_coo.cpp:123-706 (R logicals, int32 in and out)."""
    return _slice_coo_arbitrary(ii, jj, xx, MX_LGL, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq,
                                j_is_seq, i_is_rev_seq, j_is_rev_seq, nrows, ncols)


def slice_coo_arbitrary_binary(ii, jj, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq, j_is_seq,
                               i_is_rev_seq, j_is_rev_seq, nrows, ncols):
    """src/slice_coo.cpp:123-706 (pattern): dict(ii, jj, xx=None)."""
    return _slice_coo_arbitrary(ii, jj, None, MX_NONE, rows_take_base1, cols_take_base1, all_i, all_j, i_is_seq,
                                j_is_seq, i_is_rev_seq, j_is_rev_seq, nrows, ncols)


def _slice_coo_single(ii, jj, xx, vdt, i, j):
    i_, j_ = _i32(ii), _i32(jj)
    if i_.size != j_.size:
        raise ValueError("row and column indices have different length")
    v, val = None, None
    if vdt == MX_F64:
        v, val = _f64(xx), C.c_double(0.0)
    elif vdt == MX_LGL:
        v, val = np.ascontiguousarray(xx, dtype=np.int32), C.c_int32(0)
    if v is not None and v.size != i_.size:
        raise ValueError("values and indices have different number of entries")
    found = C.c_int(0)
    check(_lib.load().mx_slice_coo_single(ptr(i_), ptr(j_), ptr(v), vdt, i_.size, int(i), int(j), C.byref(found),
                                          None if val is None else C.byref(val)))
    return bool(found.value), (None if val is None else val.value)


def slice_coo_single_numeric(ii, jj, xx, i, j) -> float:
    """src/slice_coo.cpp:3-36: the value of the first triplet (storage order) at 0-based (i, j), or 0.  Duplicates
    are not summed."""
    hit, val = _slice_coo_single(ii, jj, xx, MX_F64, i, j)
    return float(val) if hit else 0.0


def slice_coo_single_logical(ii, jj, xx, i, j) -> bool:
    """src/slice_coo.cpp:38-53: the export returns a C++ bool, so the first match's NA reads as TRUE."""
    hit, val = _slice_coo_single(ii, jj, xx, MX_LGL, i, j)
    return bool(hit and val != 0)


def slice_coo_single_binary(ii, jj, i, j) -> bool:
    """src/slice_coo.cpp:55-71: TRUE when some triplet sits at (i, j)."""
    hit, _ = _slice_coo_single(ii, jj, None, MX_NONE, i, j)
    return hit


# ----------------------------------------------------------------------------- what finishes `[` (coona.hip): NA
#                                                       injection, the CSR scalar lookup, recycled selector indices
def _inject_NAs_inplace_coo(ii, jj, xx, vdt, rows_na, cols_na, nrows, ncols):
    i, j = _i32(ii), _i32(jj)
    v = np.ascontiguousarray(xx, dtype=np.float64 if vdt == MX_F64 else np.int32)
    if i.size != j.size or v.size != i.size:
        raise ValueError("indices and values have different number of entries")
    rn, cn = _i32(rows_na).reshape(-1), _i32(cols_na).reshape(-1)
    if rn.size == 0 and cn.size == 0:
        return {}                                   # the reference's empty list: nothing to inject
    out = _begin(_lib.load().mx_inject_NAs_inplace_coo_begin, ptr(i), ptr(j), ptr(v), vdt, i.size, ptr(rn), rn.size,
                 ptr(cn), cn.size, int(nrows), int(ncols), empty_values_dtype=v.dtype)[0]
    return dict(ii=out["indptr"], jj=out["indices"], xx=out["values"].astype(v.dtype, copy=False))


def inject_NAs_inplace_coo_numeric(ii, jj, xx, rows_na_, cols_na_, nrows, ncols):
    """src/slice_coo.cpp:902-923: dict(ii, jj, xx) of the triplets that stay (storage order) followed by the NA
    block of the 0-based, ascending rows_na_ / cols_na_, every value of it NA_real_."""
    return _inject_NAs_inplace_coo(ii, jj, xx, MX_F64, rows_na_, cols_na_, nrows, ncols)


def inject_NAs_inplace_coo_logical(ii, jj, xx, rows_na_, cols_na_, nrows, ncols):
    """src/slice_coo.cpp:925-946 (R logicals, int32 in and out; the block holds NA_LOGICAL)."""
    return _inject_NAs_inplace_coo(ii, jj, xx, MX_LGL, rows_na_, cols_na_, nrows, ncols)


def _extract_single_val_csr(indptr, indices, values, vdt, row, col):
    p, j = _i32(indptr), _i32(indices)
    v, val = None, None
    if vdt == MX_F64:
        v, val = _f64(values), C.c_double(0.0)
    elif vdt == MX_LGL:
        v, val = np.ascontiguousarray(values, dtype=np.int32), C.c_int32(0)
    if v is not None and v.size != j.size:
        raise ValueError("values and indices have different number of entries")
    found = C.c_int(0)
    check(_lib.load().mx_extract_single_val_csr(ptr(p), p.size - 1, ptr(j), ptr(v), vdt, int(row), int(col),
                                                C.byref(found), None if val is None else C.byref(val)))
    return bool(found.value), (None if val is None else val.value)


def extract_single_val_csr_numeric(indptr, indices, values, row, col) -> float:
    """src/slice.cpp:737-752: the value of the first entry (storage order) of 0-based `row` at column `col`, or 0."""
    hit, val = _extract_single_val_csr(indptr, indices, values, MX_F64, row, col)
    return float(val) if hit else 0.0


def extract_single_val_csr_logical(indptr, indices, values, row, col) -> int:
    """src/slice.cpp:754-769: the export returns an int, so NA_LOGICAL comes back as it is stored."""
    hit, val = _extract_single_val_csr(indptr, indices, values, MX_LGL, row, col)
    return int(val) if hit else 0


def extract_single_val_csr_binary(indptr, indices, row, col) -> float:
    """src/slice.cpp:771-785: 1 when the row stores the column, else 0."""
    hit, _ = _extract_single_val_csr(indptr, indices, None, MX_NONE, row, col)
    return 1.0 if hit else 0.0


def repeat_indices_n_times(indices, remainder, ix_length, desired_length):
    """src/slice.cpp:636-659: `indices` shifted by ix_length per full repeat inside desired_length, then `remainder`
    shifted past them."""
    ix, rem = _i32(indices).reshape(-1), _i32(remainder).reshape(-1)
    if int(ix_length) <= 0:
        raise ValueError("ix_length must be positive")
    out = np.empty(ix.size * (int(desired_length) // int(ix_length)) + rem.size, dtype=np.int32)
    check(_lib.load().mx_repeat_indices_n_times(ptr(ix), ix.size, ptr(rem), rem.size, int(ix_length),
                                                int(desired_length), ptr(out)))
    return out


def entries_to_dense_vector(pos, values, length, logical=False):
    """as.vector() of a one-row / one-column slice (drop_slice, R/slice.R:210-236; no export of the reference's, the
    mirror's way to mxd_entries_to_dense_vector): zeros of `length` with values[k] at the distinct 0-based pos[k] —
    float64, or int32 R logicals for int32 values and, with logical=True, for no values (TRUE)."""
    ps = _i32(pos).reshape(-1)
    if values is None:
        v, vdt, odt = None, MX_NONE, MX_LGL if logical else MX_F64
    elif np.asarray(values).dtype == np.float64:
        v, vdt, odt = _f64(values), MX_F64, MX_F64
    else:
        v, vdt, odt = np.ascontiguousarray(values, dtype=np.int32), MX_LGL, MX_LGL
    if v is not None and v.size != ps.size:
        raise ValueError("values and positions have different number of entries")
    out = np.empty(int(length), dtype=np.float64 if odt == MX_F64 else np.int32)
    check(_lib.load().mx_entries_to_dense_vector(ptr(ps), ptr(v), vdt, ps.size, ptr(out), odt, out.size))
    return out


# ----------------------------------------------------------------------------- remove_sparse_zeros / filterSparse /
#                                                                               check_sparse_matrix (compact.hip)
def _compacted(res, info, inputs, vdt):
    """(indptr-or-ii, indices, values) of a compaction result: the input objects themselves when nothing was removed
    (MX_ALIAS_ALL), else the new vectors."""
    lib = _lib.load()
    if info.alias_structure == _lib.MX_ALIAS_ALL:
        lib.mx_result_discard(res)
        return inputs
    out = _finish(res, info, empty_values_dtype=vdt)
    return out["indptr"], out["indices"], out["values"].astype(vdt, copy=False)


def _remove_zeros_csr(fn, indptr, indices, values, remove_NAs, vdt):
    p, j, v = _i32(indptr), _i32(indices), np.ascontiguousarray(values, dtype=vdt)
    if j.size != v.size or p.size < 1:
        raise ValueError("indptr, indices and values do not form a CSR")
    a, b, c = _begin(fn, ptr(p), ptr(j), ptr(v), p.size - 1, int(bool(remove_NAs)), finish=_compacted,
                     inputs=(indptr, indices, values), vdt=vdt)[0]
    return dict(indptr=a, indices=b, values=c)


def remove_zero_valued_csr_numeric(indptr, indices, values, remove_NAs):
    """src/misc.cpp:667-683: dict(indptr, indices, values); the inputs themselves when nothing is removed."""
    return _remove_zeros_csr(_lib.load().mx_remove_zero_valued_csr_numeric, indptr, indices, values, remove_NAs,
                             np.float64)


def remove_zero_valued_csr_logical(indptr, indices, values, remove_NAs):
    """src/misc.cpp:684-699 (with remove_NAs only NA is removed, FALSE is kept: misc.cpp:637-648)."""
    return _remove_zeros_csr(_lib.load().mx_remove_zero_valued_csr_logical, indptr, indices, values, remove_NAs,
                             np.int32)


def _remove_zeros_coo(fn, ii, jj, xx, remove_NAs, vdt):
    i, j, v = _i32(ii), _i32(jj), np.ascontiguousarray(xx, dtype=vdt)
    if not (i.size == j.size == v.size):
        raise ValueError("ii, jj and xx have different lengths")
    a, b, c = _begin(fn, ptr(i), ptr(j), ptr(v), i.size, int(bool(remove_NAs)), finish=_compacted,
                     inputs=(ii, jj, xx), vdt=vdt)[0]
    return dict(ii=a, jj=b, xx=c)


def remove_zero_valued_coo_numeric(ii, jj, xx, remove_NAs):
    """src/misc.cpp:790-806: dict(ii, jj, xx)."""
    return _remove_zeros_coo(_lib.load().mx_remove_zero_valued_coo_numeric, ii, jj, xx, remove_NAs, np.float64)


def remove_zero_valued_coo_logical(ii, jj, xx, remove_NAs):
    """src/misc.cpp:807-822."""
    return _remove_zeros_coo(_lib.load().mx_remove_zero_valued_coo_logical, ii, jj, xx, remove_NAs, np.int32)


def _remove_zeros_svec(fn, ii, xx, remove_NAs, vdt):
    i, v = _i32(ii), np.ascontiguousarray(xx, dtype=vdt)
    if i.size != v.size:
        raise ValueError("ii and xx have different lengths")
    _, b, c = _begin(fn, ptr(i), ptr(v), i.size, int(bool(remove_NAs)), finish=_compacted,
                     inputs=(None, ii, xx), vdt=vdt)[0]
    return dict(ii=b, xx=c)


def remove_zero_valued_svec_numeric(ii, xx, remove_NAs):
    """src/misc.cpp:925-938 (with remove_NAs NaN is still kept: misc.cpp:882-886)."""
    return _remove_zeros_svec(_lib.load().mx_remove_zero_valued_svec_numeric, ii, xx, remove_NAs, np.float64)


def remove_zero_valued_svec_integer(ii, xx, remove_NAs):
    """src/misc.cpp:940-953."""
    return _remove_zeros_svec(_lib.load().mx_remove_zero_valued_svec_integer, ii, xx, remove_NAs, np.int32)


def remove_zero_valued_svec_logical(ii, xx, remove_NAs):
    """src/misc.cpp:955-968."""
    return _remove_zeros_svec(_lib.load().mx_remove_zero_valued_svec_logical, ii, xx, remove_NAs, np.int32)


def _filter(layout, indptr, idx0, idx1, values, mask):
    v, vd = _values_kind(values)
    if v is None:
        raise TypeError("filtering needs values")
    i0 = _i32(idx0)
    i1 = None if idx1 is None else _i32(idx1)
    mk = _i32(mask)
    if mk.size != i0.size or v.size != i0.size or (i1 is not None and i1.size != i0.size):
        raise ValueError("mask, indices and values have different lengths")
    p = None if indptr is None else _i32(indptr)
    return _begin(_lib.load().mx_filter_sparse_begin, layout, ptr(p), 0 if p is None else p.size - 1, ptr(i0), ptr(i1),
                  ptr(v), vd, i0.size, ptr(mk), finish=_compacted, inputs=None, vdt=v.dtype)[0]


def filter_csr(indptr, indices, values, mask):
    """filterSparse of a CSR / CSC (R/utils.R:655-674): keeps entry k where the R-logical mask[k] is TRUE or NA (NA
    writes NA_real_ / NA_LOGICAL as its value); the indptr is rebuilt as rebuild_indptr_after_filter does."""
    a, b, c = _filter(0, indptr, indices, None, values, mask)
    return dict(indptr=a, indices=b, values=c)


def filter_coo(ii, jj, xx, mask):
    """filterSparse of a COO (R/utils.R:628-637)."""
    a, b, c = _filter(1, None, ii, jj, xx, mask)
    return dict(ii=a, jj=b, xx=c)


def rebuild_indptr_after_filter(indptr, filter):
    """src/misc.cpp:1099-1116: the indptr after dropping the entries whose R-logical filter is FALSE (0)."""
    p, f = _i32(indptr), _i32(filter)
    out = np.empty(p.size, dtype=np.int32)
    check(_lib.load().mx_rebuild_indptr_after_filter(ptr(p), p.size, ptr(f), ptr(out)))
    return out


def _err(e):
    return {} if e.value is None else dict(err=e.value.decode())


def check_valid_csr_matrix(indptr, indices, nrows, ncols):
    """src/misc.cpp:970-1017: {} when valid, else dict(err=<the reference's message of the first failing check>)."""
    p, j = _i32(indptr), _i32(indices)
    e = C.c_char_p()
    check(_lib.load().mx_check_valid_csr_matrix(ptr(p), p.size, ptr(j), j.size, int(nrows), int(ncols), C.byref(e)))
    return _err(e)


def check_valid_coo_matrix(ii, jj, nrows, ncols):
    """src/misc.cpp:1018-1068."""
    i, j = _i32(ii), _i32(jj)
    if i.size != j.size:
        raise ValueError("ii and jj have different lengths")
    e = C.c_char_p()
    check(_lib.load().mx_check_valid_coo_matrix(ptr(i), ptr(j), i.size, int(nrows), int(ncols), C.byref(e)))
    return _err(e)


def check_valid_svec(ii, nrows):
    """src/misc.cpp:1069-1097 (the R caller passes the 1-based @i and the length)."""
    i = _i32(ii)
    e = C.c_char_p()
    check(_lib.load().mx_check_valid_svec(ptr(i), i.size, int(nrows), C.byref(e)))
    return _err(e)


# ----------------------------------------------------------------------------- dense matrix * sparse vector, COO * dense matrix (densevec.hip)
def dense_by_svec_route(nrows, ncols, length) -> int:
    """mx_dense_by_svec_route: MX_DSV_ROUTE_A / _D (dense result) or _B / _C (CSR result), src/operators.cpp:3720-4235."""
    route = _lib.load().mx_dense_by_svec_route(int(nrows), int(ncols), int(length))
    if route < 0:
        check(1)
    return route


def _dense_by_svec(kind, X_, ii, xx, length, keep_NAs):
    X, vi, vx = _dense(X_, _CSC_DENSE_DT[kind]), _i32(ii), _f64(xx)
    if vx.size != vi.size:
        raise ValueError("ii and xx have different lengths")
    lib = _lib.load()
    args = (ptr(X), kind, X.shape[0], X.shape[1], ptr(vi), ptr(vx), vi.size, int(length), int(bool(keep_NAs)))
    if dense_by_svec_route(X.shape[0], X.shape[1], length) in (_lib.MX_DSV_ROUTE_B, _lib.MX_DSV_ROUTE_C):
        return _begin(lib.mx_multiply_elemwise_dense_by_svec_begin, *args)[0]
    out = np.empty(X.shape, dtype=np.float64, order="F")
    check(lib.mx_multiply_elemwise_dense_by_svec_dense(*args, ptr(out)))
    return dict(X_dense=out)


def multiply_elemwise_dense_by_svec_numeric(X_, ii, xx, length, keep_NAs):
    """src/operators.cpp:4305-4322: dict(X_dense=...) (F-order f64) when the vector covers the cells, or recycles over
    them unevenly; dict(indptr, indices, values), a CSR of full rows, when its length divides the number of rows.  `ii`
    holds 1-based positions, sorted when keep_NAs is set."""
    return _dense_by_svec(0, X_, ii, xx, length, keep_NAs)


def multiply_elemwise_dense_by_svec_integer(X_, ii, xx, length, keep_NAs):
    """src/operators.cpp:4324-4341 (NA cells: NA_INTEGER)."""
    return _dense_by_svec(2, X_, ii, xx, length, keep_NAs)


def multiply_elemwise_dense_by_svec_logical(X_, ii, xx, length, keep_NAs):
    """src/operators.cpp:4343-4360: R logical X (int32 or bool), read as integers."""
    return _dense_by_svec(3, X_, ii, xx, length, keep_NAs)


def multiply_elemwise_dense_by_svec_float32(X_, ii, xx, length, keep_NAs):
    """src/operators.cpp:4362-4379: X_ holds the float32 values (float32@Data), widened to f64 per cell."""
    return _dense_by_svec(1, X_, ii, xx, length, keep_NAs)


def _coo_by_dense(fn, kind, X_, Y_coo_row, Y_coo_col, Y_coo_val):
    X, i, j = _dense(X_, _CSC_DENSE_DT[kind]), _i32(Y_coo_row), _i32(Y_coo_col)
    xv = np.ascontiguousarray(Y_coo_val, dtype=np.int32 if kind == 4 else np.float64)
    if not i.size == j.size == xv.size:
        raise ValueError("row, col and val have different lengths")
    out = np.empty(xv.size, dtype=xv.dtype)
    check(fn(ptr(X), X.shape[0], X.shape[1], ptr(i), ptr(j), ptr(xv), xv.size, ptr(out)))
    return dict(row=i.copy(), col=j.copy(), val=out)         # new row / col vectors, as :763-769


def multiply_coo_by_dense_numeric(X_, Y_coo_row, Y_coo_col, Y_coo_val):
    """src/operators.cpp:772-787: dict(row, col, val) with val[k] = Y_coo_val[k] * X_[row[k], col[k]]."""
    return _coo_by_dense(_lib.load().mx_multiply_coo_by_dense_numeric, 0, X_, Y_coo_row, Y_coo_col, Y_coo_val)


def multiply_coo_by_dense_integer(X_, Y_coo_row, Y_coo_col, Y_coo_val):
    """src/operators.cpp:789-804: an NA_INTEGER cell gives NA_real_."""
    return _coo_by_dense(_lib.load().mx_multiply_coo_by_dense_integer, 2, X_, Y_coo_row, Y_coo_col, Y_coo_val)


def multiply_coo_by_dense_logical(X_, Y_coo_row, Y_coo_col, Y_coo_val):
    """src/operators.cpp:806-821: R logical X_ (int32 or bool) read as bool; NA gives NA_real_."""
    return _coo_by_dense(_lib.load().mx_multiply_coo_by_dense_logical, 3, X_, Y_coo_row, Y_coo_col, Y_coo_val)


def multiply_coo_by_dense_float32(X_, Y_coo_row, Y_coo_col, Y_coo_val):
    """src/operators.cpp:823-838: X_ holds the float32 values (float32@Data)."""
    return _coo_by_dense(_lib.load().mx_multiply_coo_by_dense_float32, 1, X_, Y_coo_row, Y_coo_col, Y_coo_val)


def logicaland_coo_by_dense_logical(X_, Y_coo_row, Y_coo_col, Y_coo_val):
    """src/operators.cpp:840-855: R logicals in and out, R's three-valued AND."""
    return _coo_by_dense(_lib.load().mx_logicaland_coo_by_dense_logical, 4, X_, Y_coo_row, Y_coo_col, Y_coo_val)


# ----------------------------------------------------------------------------- `[<-` of a dgRMatrix (assign.hip)
_SEL_ALL, _SEL_SINGLE, _SEL_RANGE, _SEL_ARBITRARY = (_lib.MX_SEL_ALL, _lib.MX_SEL_SINGLE, _lib.MX_SEL_RANGE,
                                                     _lib.MX_SEL_ARBITRARY)
_ALL = (_SEL_ALL, 0, 0, None)
# the zero-route exports of the reference take no ncol, and the zero route needs none
_NCOL_UNKNOWN = 2**31 - 1


def _one(k):
    return (_SEL_SINGLE, int(k), int(k), None)


def _seq(lo, hi):
    return (_SEL_RANGE, int(lo), int(hi), None)


def _arb(idx):
    return (_SEL_ARBITRARY, 0, 0, _i32(idx))


def _assigned(res, info, inputs):
    """dict(indptr, indices, values) of an assignment: the input objects themselves (MX_ALIAS_ALL), the input indptr
    and indices with new values (alias 1), or three new vectors, as the reference's export returns them."""
    if info.alias_structure == _lib.MX_ALIAS_ALL:
        check(_lib.load().mx_result_discard(res))
        return dict(indptr=inputs[0], indices=inputs[1], values=inputs[2])
    return _finish(res, info, alias_from=inputs[:2])


def rows_are_sorted(p, j):
    """Host check: every row's column indices strictly ascend."""
    p, j = np.asarray(p), np.asarray(j)
    back = np.flatnonzero(j[1:] <= j[:-1]) + 1          # entries not above their predecessor: row starts only
    return bool(np.isin(back, p).all())


def _assign_scalar(indptr, indices, values, ncols, sel_i, sel_j, value):
    p, j, v = _i32(indptr), _i32(indices), _f64(values)
    if j.size != v.size or p.size < 1:
        raise ValueError("indptr, indices and values do not form a CSR")
    (ki, ilo, ihi, rows), (kj, jlo, jhi, cols) = sel_i, sel_j
    return _begin(_lib.load().mx_assign_csr_scalar_begin, ptr(p), p.size - 1, ptr(j), ptr(v), int(ncols),
                  ki, ilo, ihi, ptr(rows), 0 if rows is None else rows.size,
                  kj, jlo, jhi, ptr(cols), 0 if cols is None else cols.size, float(value),
                  finish=_assigned, inputs=(indptr, indices, values))[0]


def _assign_rows(indptr, indices, values, sel_i, indptr_other, indices_other, values_other):
    p, j, v = _i32(indptr), _i32(indices), _f64(values)
    vp, vj, vv = _i32(indptr_other), _i32(indices_other), _f64(values_other)
    if j.size != v.size or p.size < 1 or vj.size != vv.size or vp.size < 1:
        raise ValueError("indptr, indices and values do not form a CSR")
    ki, ilo, ihi, rows = sel_i
    return _begin(_lib.load().mx_assign_csr_rows_begin, ptr(p), p.size - 1, ptr(j), ptr(v), ki, ilo, ihi, ptr(rows),
                  0 if rows is None else rows.size, ptr(vp), vp.size - 1, ptr(vj), ptr(vv),
                  finish=_assigned, inputs=(indptr, indices, values))[0]


def set_single_row_to_zero(indptr, indices, values, row_set):
    """src/assignment.cpp:384-424."""
    return _assign_scalar(indptr, indices, values, _NCOL_UNKNOWN, _one(row_set), _ALL, 0.0)


def set_single_col_to_zero(indptr, indices, values, col_set):
    """src/assignment.cpp:426-496."""
    return _assign_scalar(indptr, indices, values, _NCOL_UNKNOWN, _ALL, _one(col_set), 0.0)


def set_single_row_to_const(indptr, indices, values, ncols, row_set, val_set):
    """src/assignment.cpp:498-559."""
    return _assign_scalar(indptr, indices, values, ncols, _one(row_set), _ALL, val_set)


def set_single_col_to_const(indptr, indices, values, ncols, col_set, val_set):
    """src/assignment.cpp:561-630."""
    return _assign_scalar(indptr, indices, values, ncols, _ALL, _one(col_set), val_set)


def set_single_val_to_zero(indptr, indices, values, row_set, col_set):
    """src/assignment.cpp:632-684."""
    return _assign_scalar(indptr, indices, values, _NCOL_UNKNOWN, _one(row_set), _one(col_set), 0.0)


def set_single_val_to_const(indptr, indices, values, ncols, row_set, col_set, val_set):
    """src/assignment.cpp:686-769."""
    return _assign_scalar(indptr, indices, values, ncols, _one(row_set), _one(col_set), val_set)


def set_rowseq_to_zero(indptr, indices, values, row_set_st, row_set_end):
    """src/assignment.cpp:1135-1171: always new vectors."""
    return _assign_scalar(indptr, indices, values, _NCOL_UNKNOWN, _seq(row_set_st, row_set_end), _ALL, 0.0)


def set_rowseq_to_const(indptr, indices, values, row_set_st, row_set_end, ncols, val_set):
    """src/assignment.cpp:1173-1233."""
    return _assign_scalar(indptr, indices, values, ncols, _seq(row_set_st, row_set_end), _ALL, val_set)


def set_colseq_to_zero(indptr, indices, values, col_set_st, col_set_end, ncols):
    """src/assignment.cpp:1235-1291."""
    return _assign_scalar(indptr, indices, values, ncols, _ALL, _seq(col_set_st, col_set_end), 0.0)


def set_colseq_to_const(indptr, indices, values, col_set_st, col_set_end, ncols, val_set):
    """src/assignment.cpp:1293-1364: always new vectors."""
    return _assign_scalar(indptr, indices, values, ncols, _ALL, _seq(col_set_st, col_set_end), val_set)


def set_arbitrary_rows_to_zero(indptr, indices, values, rows_set):
    """src/assignment.cpp:1366-1443."""
    return _assign_scalar(indptr, indices, values, _NCOL_UNKNOWN, _arb(rows_set), _ALL, 0.0)


def set_arbitrary_rows_to_const(indptr, indices, values, rows_set, ncols, val_set):
    """src/assignment.cpp:1445-1597."""
    return _assign_scalar(indptr, indices, values, ncols, _arb(rows_set), _ALL, val_set)


def set_arbitrary_cols_to_zero(indptr, indices, values, cols_set, ncols):
    """src/assignment.cpp:1599-1661."""
    return _assign_scalar(indptr, indices, values, ncols, _ALL, _arb(cols_set), 0.0)


def set_arbitrary_cols_to_const(indptr, indices, values, cols_set, ncols, val_set):
    """src/assignment.cpp:1663-1793."""
    return _assign_scalar(indptr, indices, values, ncols, _ALL, _arb(cols_set), val_set)


def set_arbitrary_rows_single_col_to_zero(indptr, indices, values, rows_set, col_set, ncols):
    """src/assignment.cpp:1795-1898."""
    return _assign_scalar(indptr, indices, values, ncols, _arb(rows_set), _one(col_set), 0.0)


def set_arbitrary_rows_single_col_to_const(indptr, indices, values, rows_set, col_set, val_set, ncols):
    """src/assignment.cpp:1900-2060."""
    return _assign_scalar(indptr, indices, values, ncols, _arb(rows_set), _one(col_set), val_set)


def set_single_row_arbitrary_cols_to_zero(indptr, indices, values, row_set, cols_set, ncols):
    """src/assignment.cpp:2062-2159."""
    return _assign_scalar(indptr, indices, values, ncols, _one(row_set), _arb(cols_set), 0.0)


def set_single_row_arbitrary_cols_to_const(indptr, indices, values, row_set, cols_set, ncols, val_set):
    """src/assignment.cpp:2161-2251."""
    return _assign_scalar(indptr, indices, values, ncols, _one(row_set), _arb(cols_set), val_set)


def set_arbitrary_rows_arbitrary_cols_to_zero(indptr, indices, values, rows_set, cols_set, ncols):
    """src/assignment.cpp:2253-2358."""
    return _assign_scalar(indptr, indices, values, ncols, _arb(rows_set), _arb(cols_set), 0.0)


def set_arbitrary_rows_arbitrary_cols_to_const(indptr, indices, values, rows_set, cols_set, ncols, val_set):
    """src/assignment.cpp:2360-2476."""
    return _assign_scalar(indptr, indices, values, ncols, _arb(rows_set), _arb(cols_set), val_set)


def set_rowseq_to_smat(indptr, indices, values, row_set_st, row_set_end, indptr_other, indices_other, values_other):
    """src/assignment.cpp:2478-2521."""
    return _assign_rows(indptr, indices, values, _seq(row_set_st, row_set_end), indptr_other, indices_other,
                        values_other)


def set_arbitrary_rows_to_smat(indptr, indices, values, rows_set, indptr_other, indices_other, values_other):
    """src/assignment.cpp:2523-2598, in any order of rows_set and without its tail defect (:2554): row rows_set[k]
    becomes row k of the other matrix."""
    return _assign_rows(indptr, indices, values, _arb(rows_set), indptr_other, indices_other, values_other)


def _assign_vec(fn, indptr, indices, values, ncols, at, ii, xx, length):
    """One row or one column <- a pattern (ii, xx, length); ii None for a dense vector."""
    p, j, v = _i32(indptr), _i32(indices), _f64(values)
    if j.size != v.size or p.size < 1:
        raise ValueError("indptr, indices and values do not form a CSR")
    xx = _f64(xx)
    ii = None if ii is None else _i32(ii)
    if ii is not None and ii.size != xx.size:
        raise ValueError("the vector's indices and values differ in length")
    # an empty sparse vector travels as n_xx = 0; a dense one as a null ii
    return _begin(fn, ptr(p), p.size - 1, ptr(j), ptr(v), int(ncols), int(at), ptr(ii), ptr(xx), xx.size, int(length),
                  finish=_assigned, inputs=(indptr, indices, values))[0]


def set_single_row_to_rowvec(indptr, indices, values, ncols, row_set, vec_set):
    """src/assignment.cpp:771-837; a full row that is not sorted gives three new vectors."""
    vec = _f64(vec_set)
    return _assign_vec(_lib.load().mx_assign_csr_row_vec_begin, indptr, indices, values, ncols, row_set, None, vec,
                       vec.size)


def set_single_col_to_colvec(indptr, indices, values, ncols, col_set, vec_set):
    """src/assignment.cpp:839-913."""
    vec = _f64(vec_set)
    return _assign_vec(_lib.load().mx_assign_csr_col_vec_begin, indptr, indices, values, ncols, col_set, None, vec,
                       vec.size)


def set_single_row_to_svec(indptr, indices, values, ncols, row_set, ii, xx, length):
    """src/assignment.cpp:915-1007, ii 0-based in any order; without the two defects of its fast path (:939-966)."""
    return _assign_vec(_lib.load().mx_assign_csr_row_vec_begin, indptr, indices, values, ncols, row_set, _i32(ii), xx,
                       length)


def set_single_col_to_svec(indptr, indices, values, ncols, col_set, ii, xx, length):
    """src/assignment.cpp:1009-1133, ii 0-based and ascending: always new vectors."""
    return _assign_vec(_lib.load().mx_assign_csr_col_vec_begin, indptr, indices, values, ncols, col_set, _i32(ii), xx,
                       length)


# ----------------------------------------------------------------------------- reductions (include/mxgpu_reduce.h)
def _csr_values(values, value_dtype):
    """(values array or None, mx_dtype) of a CSR operand's @x: float64, int32 R logicals, or None for a pattern."""
    if values is None:
        return None, MX_NONE
    if value_dtype is None:
        value_dtype = MX_LGL if np.asarray(values).dtype == np.int32 else MX_F64
    return (_i32(values) if value_dtype == MX_LGL else _f64(values)), value_dtype


def _csr_operand(indptr, indices, values, value_dtype):
    p, j = _i32(indptr), _i32(indices)
    x, vd = _csr_values(values, value_dtype)
    if p.size < 1 or int(p[-1]) != j.size or (x is not None and x.size != j.size):
        raise ValueError("indptr, indices and values do not form a CSR")
    return p, j, x, vd


def csr_margin_reduce(indptr, indices, values, ncols, axis, op=_lib.MX_RED_SUM, na_rm=False, mean=False,
                      value_dtype=None):
    """mx_csr_margin_reduce: `op` (an mx_reduce_op) over the rows (axis 0) or the columns (axis 1) of a CSR with
    `ncols` columns, as float64[nrow or ncol]; mean=True divides by the other dimension, less the NAs na_rm skipped."""
    p, j, x, vd = _csr_operand(indptr, indices, values, value_dtype)
    nrow, ncol = p.size - 1, int(ncols)
    out = np.empty(nrow if int(axis) == 0 else ncol, dtype=np.float64)
    check(_lib.load().mx_csr_margin_reduce(nrow, ncol, ptr(p), ptr(j), ptr(x), vd, int(axis), int(op), int(bool(na_rm)),
                                           int(bool(mean)), ptr(out)))
    return out


def csr_norm(indptr, indices, values, ncols, type, value_dtype=None):
    """mx_csr_norm: type one of "O", "I", "F", "M" (norm_csr, R/csr_linalg.R:13-31), as a float."""
    p, j, x, vd = _csr_operand(indptr, indices, values, value_dtype)
    out = np.zeros(1, dtype=np.float64)
    check(_lib.load().mx_csr_norm(p.size - 1, int(ncols), ptr(p), ptr(j), ptr(x), vd, ord(type), ptr(out)))
    return float(out[0])


def csr_diag(indptr, indices, values, ncols, value_dtype=None):
    """mx_csr_diag: the first stored (k, k) of every row k < min(nrow, ncol), 0 where there is none; float64 for
    numeric values, int32 R logicals for logical values (NA kept) and for a pattern (0 / 1)."""
    p, j, x, vd = _csr_operand(indptr, indices, values, value_dtype)
    out = np.empty(min(p.size - 1, int(ncols)), dtype=np.float64 if vd == MX_F64 else np.int32)
    check(_lib.load().mx_csr_diag(p.size - 1, int(ncols), ptr(p), ptr(j), ptr(x), vd, ptr(out)))
    return out


# ----------------------------------------------------------------------------- transposed products (include/mxgpu_tprod.h)
def csr_tmatvec(indptr, indices, values, ncols, v):
    """mx_csr_tmatvec: X^T v for a CSR X with `ncols` columns (values float64, or None for a pattern) and a float64 v of
    nrow elements, as float64[ncols]."""
    p, j, x, vd = _csr_operand(indptr, indices, values, None if values is None else MX_F64)
    v = _f64(v).reshape(-1)
    nrow, ncol = p.size - 1, int(ncols)
    if v.size != nrow:
        raise ValueError("csr_tmatvec: v must have one element per row of X")
    out = np.empty(ncol, dtype=np.float64)
    check(_lib.load().mx_csr_tmatvec(nrow, ncol, ptr(p), ptr(j), ptr(x), vd, ptr(v), ptr(out)))
    return out


def csr_tmatmul_dense(indptr, indices, values, ncols, B_rowmajor, colmajor_out=True):
    """mx_csr_tmatmul_dense: X^T B for a CSR X with `ncols` columns and float64 values, B a C-contiguous nrow x n
    float64 / float32 array: an ncols x n array of B's type, column-major (Fortran order) with colmajor_out, else
    row-major."""
    p, j, x, _ = _csr_operand(indptr, indices, values, MX_F64)
    B = np.asarray(B_rowmajor)
    if B.ndim != 2 or B.dtype not in (np.float64, np.float32):
        raise ValueError("csr_tmatmul_dense: B must be a 2-d float64 / float32 array")
    B = np.ascontiguousarray(B)
    nrow, ncol, n = p.size - 1, int(ncols), B.shape[1]
    if B.shape[0] != nrow:
        raise ValueError("csr_tmatmul_dense: B must have one row per row of X")
    out = np.empty((ncol, n), dtype=B.dtype, order="F" if colmajor_out else "C")
    check(_lib.load().mx_csr_tmatmul_dense(nrow, ncol, ptr(p), ptr(j), ptr(x), ptr(B), n, n,
                                           MX_F64 if B.dtype == np.float64 else _lib.MX_F32, ptr(out),
                                           ncol if colmajor_out else n, int(bool(colmajor_out))))
    return out


# ----------------------------------------------------------------------------- sparse x sparse (include/mxgpu_spgemm.h)
def csr_spgemm(p1, j1, x1, dims1, trans_a, p2, j2, x2, dims2, trans_b):
    """mx_csr_spgemm_begin: op(A) op(B) for the CSR arrays of A (dims1 = (nrow, ncol); values float64, int32 R logicals
    or None for a pattern) and of B, op(X) = t(X) where trans_a / trans_b is set, as dict(indptr, indices, values) of
    the CSR of the product: float64 values, rows sorted, nothing dropped.  One upload and one download; a transpose is
    made on the device."""
    pa, ja, xa, va = _csr_operand(p1, j1, x1, None)
    pb, jb, xb, vb = _csr_operand(p2, j2, x2, None)
    (m, K), (K2, n) = (int(d) for d in dims1), (int(d) for d in dims2)
    if pa.size != m + 1 or pb.size != K2 + 1:
        raise ValueError("csr_spgemm: indptr and dims disagree")
    return _begin(_lib.load().mx_csr_spgemm_begin, ptr(pa), m, K, ptr(ja), ptr(xa), va, int(bool(trans_a)), ptr(pb), K2, n,
                  ptr(jb), ptr(xb), vb, int(bool(trans_b)))[0]


# ----------------------------------------------------------------------------- structured operands (include/mxgpu_sym.h)
_UPLO = {"U": _lib.MX_UPLO_UPPER, "L": _lib.MX_UPLO_LOWER}


def _uplo(uplo):
    if uplo not in _UPLO:
        raise ValueError("Matrix has invalid 'uplo' field.")
    return _UPLO[uplo]


def _structured_begin(fn, indptr, indices, values, uplo, value_dtype):
    p, j, x, vd = _csr_operand(indptr, indices, values, value_dtype)
    out = _begin(fn, ptr(p), p.size - 1, ptr(j), ptr(x), vd, 0 if x is None else x.size, _uplo(uplo),
                 empty_values_dtype=np.float64 if x is None else x.dtype)[0]
    out["values"] = None if x is None else out["values"].astype(x.dtype, copy=False)
    return out


def csr_symmetric_to_general(indptr, indices, values, uplo, value_dtype=None):
    """mx_csr_symmetric_to_general_begin: the general CSR of an n x n symmetric CSR that stores the triangle `uplo`
    ("U" / "L"), Matrix's as(x, "generalMatrix") behind as.csr.matrix of a dsR / lsR / nsR (R/conversions.R:180-295);
    a dsC's (p, i, x) with uplo flipped gives its general CSC arrays.  Row r of the result is the mirrored entries and
    the stored row (U: mirrored first, L: stored first); values are copied bit for bit.  values None -> a pattern."""
    return _structured_begin(_lib.load().mx_csr_symmetric_to_general_begin, indptr, indices, values, uplo, value_dtype)


def csr_unit_triangular_to_general(indptr, indices, values, uplo, value_dtype=None):
    """mx_csr_unit_triangular_to_general_begin: the general CSR of a triangular CSR with diag = "U": every row gains
    (r, r) = 1.0 / TRUE / pattern, in front of the stored row (U) or behind it (L).  An entry on the diagonal or in
    the other triangle is an error."""
    return _structured_begin(_lib.load().mx_csr_unit_triangular_to_general_begin, indptr, indices, values, uplo,
                             value_dtype)


def csr_triangle_check(indptr, indices, uplo, strict=False):
    """mx_csr_triangle_check: how many entries of the square CSR lie outside the triangle `uplo` (strict: or on the
    diagonal)."""
    p, j = _i32(indptr), _i32(indices)
    out = C.c_int64(0)
    check(_lib.load().mx_csr_triangle_check(ptr(p), p.size - 1, ptr(j), _uplo(uplo), int(bool(strict)), C.byref(out)))
    return int(out.value)


# ----------------------------------------------------------------------------- one-triangle Gram product (mxgpu_gram.h)
def csr_gram(indptr, indices, values, dims, trans, uplo):
    """mx_csr_gram_begin: the triangle `uplo` ("U" / "L") of X X^T (trans false) or X^T X (trans true) for the CSR
    arrays of X (dims = (nrow, ncol); values float64, int32 R logicals or None for a pattern), as dict(indptr, indices,
    values) of a CSR that stores that triangle alone: float64 values, rows sorted, nothing dropped.  One upload and one
    download; the transpose is made on the device.  With sorted rows of X the other triangle of the full product holds
    the same bits."""
    p, j, x, vd = _csr_operand(indptr, indices, values, None)
    nrow, ncol = (int(d) for d in dims)
    if p.size != nrow + 1:
        raise ValueError("csr_gram: indptr and dims disagree")
    return _begin(_lib.load().mx_csr_gram_begin, ptr(p), nrow, ncol, ptr(j), ptr(x), vd, int(bool(trans)), _uplo(uplo))[0]


# ----------------------------------------------------------------------------- dense <-> compressed (mxgpu_dense.h)
_DENSE_KINDS = {np.dtype(np.float64): MX_F64, np.dtype(np.float32): _lib.MX_F32, np.dtype(np.int32): _lib.MX_I32}


def dense_to_csr(dense, by_col=False, out_dtype=MX_F64):
    """mx_dense_to_csr_begin: the CSR arrays (by_col: the CSC arrays) of a dense 2-d array as dict(indptr, indices,
    values): the cells that are not zero, NaN and NA kept, -0.0 dropped, rows sorted.  float64 and float32 arrays are
    numeric, int32 arrays R integers, bool arrays R logicals.  out_dtype MX_F64: float64 values (NA_integer_ ->
    NA_real_); MX_LGL: int32 R logicals (NaN -> NA, any other kept cell TRUE); MX_NONE: `values` is None."""
    M = np.asarray(dense)
    if M.ndim != 2:
        raise ValueError("dense operand must be a 2-d matrix")
    if out_dtype not in (MX_F64, MX_LGL, MX_NONE):
        raise ValueError("dense_to_csr: out_dtype must be MX_F64, MX_LGL or MX_NONE")
    if M.dtype == np.bool_:
        M, kind = np.asfortranarray(M, dtype=np.int32), MX_LGL
    elif M.dtype in _DENSE_KINDS:
        M, kind = np.asfortranarray(M), _DENSE_KINDS[M.dtype]
    else:
        raise TypeError(f"dense operand must be float64, float32, int32 or bool, got {M.dtype}")
    out = _begin(_lib.load().mx_dense_to_csr_begin, ptr(M), M.shape[0], M.shape[1], kind, int(bool(by_col)),
                 int(out_dtype), empty_values_dtype=np.int32 if out_dtype == MX_LGL else np.float64)[0]
    if out_dtype == MX_NONE:
        out["values"] = None
    return out


def csr_to_dense(indptr, indices, values, nother, by_col=False, logical=False):
    """mx_csr_to_dense: the CSR arrays of an nrow x `nother` matrix (by_col: the CSC arrays of an `nother` x ncol one;
    values float64, int32 R logicals or None for a pattern) as a dense column-major array: float64 (NA -> NA_real_, a
    pattern entry -> 1.0), or int32 R logicals with `logical`.  Unsorted rows and repeated cells are normalised on the
    device first (repeated cells merged as coo_to_csr merges them); an index out of bounds is an error."""
    p, j, x, vd = _csr_operand(indptr, indices, values, None)
    nseg, nother = p.size - 1, int(nother)
    shape = (nother, nseg) if by_col else (nseg, nother)
    out = np.empty(shape, dtype=np.int32 if logical else np.float64, order="F")
    check(_lib.load().mx_csr_to_dense(ptr(p), nseg, nother, ptr(j), ptr(x), vd, int(bool(by_col)), ptr(out),
                                      MX_LGL if logical else MX_F64))
    return out
