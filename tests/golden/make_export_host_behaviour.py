#!/usr/bin/env python3
"""Generates tests/golden/export_host_behaviour.json: what every mx_* export defined in csrc/api.hip does BEFORE its
first device call.  For each function there is one call that trips each argument check (MX_REQUIRE / set_error)
evaluated before the first device call, with every earlier check passing, and one call for each return of status 0
taken before it (no rows, no cells, the zeroed C of an SpMM with nothing to multiply, the zeroed `out` of
mx_matmul_csr_svec with an empty vector, no entries, fewer than two indices, the end-point negative of
mx_check_is_seq / mx_check_is_rev_seq, all four routes and the -1 of mx_dense_by_svec_route).  An entry holds the
call, the status, the text of mx_last_error() for a non-zero status, and the bytes of every output buffer, which is
pre-filled with a sentinel so that "untouched" and "zeroed" differ.  None of this needs a device, so the record
replays alike with and without one.  Arrays have at most 8 elements.

The record was taken ONCE, from the library built at the commit before the export layer got its typed device arrays
and mx_result its shaping members (csrc/api.hip), and is what tests/test_export_host_behaviour.py holds every later
build to.  Do not regenerate it from the code under test; a new export is recorded when it is added and left alone
afterwards (run with its name to add only that one).

Left out, because they can only be reached after a device call (an upload or a count pass), so that their outcome
depends on a device being there:
  - "cbind result exceeds R's int32 index range" (after both operands went up);
  - "mx_multiply_csr_by_dvec_with_NAs_begin: repeated new cells" (after the COO -> CSR of the new cells);
  - the row-index check of mx_matmul_rowvec_by_csc (after the CSC went up);
  - the `A.nnz == 0` returns of the values-only exports, "csc (.) dense: entries in a matrix without rows",
    "csr (op) vector: empty vector" and the `A.nnz < 2` return of mx_sort_sparse_indices (the number of entries is
    read after the upload);
  - the "CSR upload" checks of a second operand, and of a first one where the export's own checks already ask the
    same of the index pointer;
  - the empty selector / no entries return of mx_slice_coo_arbitrary_begin and every other success of a *_begin
    export, which ends with a synchronisation of the null stream;
  - the column-axis checks of mx_slice_coo_arbitrary_begin behind a row axis that needs its map on the device;
  - "out of host memory", and every MX_HIP failure.
Run from the repo root:  python tests/golden/make_export_host_behaviour.py [function ...]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from export_calls import run_call  # noqa: E402
from make_export_result_shapes import D, F, I, F32, F64, I32, LGL, NONE  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "export_host_behaviour.json")
INT_MAX = 2**31 - 1
RES, INFO = ["out", 8], ["out", 32]           # the mx_result ** and the mx_result_info *, as plain sentinel bytes
P2, J2, X2, L2 = I(0, 1, 2), I(0, 1), D(1.0, 2.0), I(1, 0)      # two rows, one entry each
PE = I(0, 0, 0)                                                  # two empty rows
PNEG = I(0, -1)                                                  # one row, a negative last index pointer
PBAD = I(1, 1, 2)                                                # does not start at 0
E0 = I()

CALLS = []


def call(fn, *args):
    CALLS.append([fn, list(args)])


def out(n):
    return ["out", n]


call("mx_device_count", None)
# ---- SpMM exports: negative dimension; no cells; nothing to multiply (zeroed C)
for sfx, mk, eb in (("numeric", D, 8), ("float32", F, 4)):
    Y = mk(1.0, 2.0, 3.0, 4.0)
    fn = "mx_tcrossprod_csr_dense_" + sfx               # (Xp, Xj, Xx, nrows_X, Y, nrow_Y, ncol_Y, nthreads, out)
    call(fn, P2, J2, X2, -1, Y, 2, 2, 1, out(40))
    call(fn, I(0), E0, D(), 0, Y, 2, 2, 1, out(40))
    call(fn, P2, J2, X2, 2, Y, 0, 2, 1, out(40))
    call(fn, PE, E0, D(), 2, Y, 2, 2, 1, out(40))
    fn = "mx_matmul_dense_csc_" + sfx                   # (X, nrows_X, ncols_X, Yp, Yj, Yx, ncols_Y, nthreads, out)
    call(fn, Y, 2, -1, P2, J2, X2, 2, 1, out(40))
    call(fn, Y, 0, 2, P2, J2, X2, 2, 1, out(40))
    call(fn, Y, 2, 2, I(0), E0, D(), 0, 1, out(40))
    call(fn, Y, 2, 2, PE, E0, D(), 2, 1, out(40))
    fn = "mx_tcrossprod_dense_csr_" + sfx               # (X, nrows_X, ncols_X, Yp, Yj, Yx, nrows_Y, nthreads, ncols_Y, out)
    call(fn, Y, -1, 2, P2, J2, X2, 2, 1, 2, out(40))
    call(fn, Y, 0, 2, P2, J2, X2, 2, 1, 2, out(40))
    call(fn, Y, 2, 2, I(0), E0, D(), 0, 1, 2, out(40))
    call(fn, Y, 2, 2, PE, E0, D(), 2, 1, 2, out(40))
# ---- SpMV exports (p, j, x, nrows, y, len_y, nthreads, out)
for sfx, y in (("numeric", D(1.0, 2.0)), ("integer", I(1, 2)), ("logical", I(1, 0)), ("float32", F(1.0, 2.0))):
    call("mx_matmul_csr_dvec_" + sfx, P2, J2, X2, 2, y, -1, 1, out(16))
    call("mx_matmul_csr_dvec_" + sfx, P2, J2, X2, -1, y, 2, 1, out(16))
    call("mx_matmul_csr_dvec_" + sfx, I(0), E0, D(), 0, y, 2, 1, out(16))
# ---- mx_csr_elemwise_begin(op, nrows, p1, p2, j1, j2, x1, x2, nnz1, nnz2, res, info)
fn = "mx_csr_elemwise_begin"
call(fn, 0, 2, P2, P2, J2, J2, X2, X2, 2, 2, None, INFO)
call(fn, 0, 2, P2, P2, J2, J2, X2, X2, 2, 2, RES, None)
call(fn, 6, 2, P2, P2, J2, J2, X2, X2, 2, 2, RES, INFO)
call(fn, -1, 2, P2, P2, J2, J2, X2, X2, 2, 2, RES, INFO)
call(fn, 0, -1, P2, P2, J2, J2, X2, X2, 2, 2, RES, INFO)
call(fn, 0, 2, P2, P2, J2, J2, X2, X2, -1, 2, RES, INFO)
call(fn, 0, 2, P2, P2, J2, J2, X2, X2, 2, -1, RES, INFO)
call(fn, 0, 2, None, P2, J2, J2, X2, X2, 2, 2, RES, INFO)         # CSR upload: bad arguments
call(fn, 0, 1, PNEG, PNEG, J2, J2, X2, X2, 2, 2, RES, INFO)       # CSR upload: negative index pointer
call(fn, 0, 1, I(-1, 0), PNEG, J2, J2, X2, X2, 2, 2, RES, INFO)
# ---- the CSR slices: (p, nrows, j, x, dtype, n_values, rows_take, n_take, ...)
fn = "mx_copy_csr_rows_begin"
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, None, INFO)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, RES, None)
call(fn, P2, -1, J2, X2, F64, 2, I(1), 1, RES, INFO)
call(fn, P2, 2, J2, X2, F64, 2, I(1), -1, RES, INFO)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 2**31, RES, INFO)
call(fn, P2, 2, J2, X2, I32, 2, I(1), 1, RES, INFO)
call(fn, P2, 2, J2, X2, F32, 2, I(1), 1, RES, INFO)
call(fn, None, 2, J2, X2, F64, 2, I(1), 1, RES, INFO)
call(fn, PNEG, 1, J2, X2, F64, 2, I(0), 1, RES, INFO)
fn = "mx_copy_csr_rows_col_seq_begin"                   # (..., cols_take, n_cols_take, index1, res, info)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, I(0, 1), 2, 0, None, INFO)
call(fn, P2, -1, J2, X2, F64, 2, I(1), 1, I(0, 1), 2, 0, RES, INFO)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, I(0, 1), 0, 0, RES, INFO)
call(fn, P2, 2, J2, X2, 5, 2, I(1), 1, I(0, 1), 2, 0, RES, INFO)
call(fn, None, 2, J2, X2, F64, 2, I(1), 1, I(0, 1), 2, 1, RES, INFO)
call(fn, PNEG, 1, J2, X2, LGL, 2, I(0), 1, I(0, 1), 2, 0, RES, INFO)
fn = "mx_copy_csr_arbitrary_begin"                      # (..., cols_take, n_cols_take, res, info)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, I(1, 0), 2, RES, None)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, I(1, 0), -1, RES, INFO)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, I(1, 0), 2**31, RES, INFO)
call(fn, P2, 2, J2, X2, -1, 2, I(1), 1, I(1, 0), 2, RES, INFO)
call(fn, P2, 2, J2, X2, F64, 2, I(1), 1, I(1, -1), 2, RES, INFO)
call(fn, None, 2, J2, X2, F64, 2, I(1), 1, I(1, 0), 2, RES, INFO)
call(fn, PNEG, 1, J2, X2, NONE, 0, I(0), 1, I(1, 0), 2, RES, INFO)
fn = "mx_reverse_rows_begin"                            # (p, nrows, j, x, dtype, n_values, res, info)
call(fn, P2, 2, J2, X2, F64, 2, None, INFO)
call(fn, P2, -1, J2, X2, F64, 2, RES, INFO)
call(fn, None, 2, J2, X2, F64, 2, RES, INFO)
call(fn, PNEG, 1, J2, X2, F64, 2, RES, INFO)
fn = "mx_reverse_columns_inplace"                       # (p, nrows, j, x, dtype, n_values, ncol)
call(fn, P2, 0, out(8), out(16), F64, 2, 2)
call(fn, P2, -3, out(8), out(16), F64, 2, 2)
call(fn, None, 2, out(8), out(16), F64, 2, 2)
call(fn, PNEG, 1, out(8), out(16), F64, 2, 2)
# ---- mx_matmul_csr_svec(Xp, Xj, Xx, nrows, yi, ny, yv, kind, nthreads, out)
fn = "mx_matmul_csr_svec"
call(fn, P2, J2, X2, -1, I(1), 1, D(1.0), 0, 1, out(24))
call(fn, P2, J2, X2, 2, I(1), -1, D(1.0), 0, 1, out(24))
call(fn, P2, J2, X2, 2, I(1), 2**31, D(1.0), 0, 1, out(24))
call(fn, P2, J2, X2, 2, I(1), 1, D(1.0), 5, 1, out(24))
call(fn, I(0), E0, D(), 0, I(1), 1, D(1.0), 0, 1, out(24))
call(fn, P2, J2, X2, 2, None, 0, None, 0, 1, out(24))
call(fn, None, J2, X2, 2, I(1), 1, D(1.0), 0, 1, out(24))
call(fn, PNEG, J2, X2, 1, I(1), 1, D(1.0), 0, 1, out(24))
# ---- mx_multiply_csr_by_dense_elemwise(p, j, x, nrows, dense, ncols, kind, values_out)
fn = "mx_multiply_csr_by_dense_elemwise"
call(fn, P2, J2, X2, -1, D(1, 2, 3, 4), 2, 0, out(16))
call(fn, P2, J2, X2, 2, D(1, 2, 3, 4), -1, 0, out(16))
call(fn, P2, J2, X2, 2, D(1, 2, 3, 4), 2, 5, out(16))
call(fn, I(0), E0, D(), 0, D(), 2, 0, out(16))
call(fn, None, J2, X2, 2, D(1, 2, 3, 4), 2, 0, out(16))
call(fn, PNEG, J2, X2, 1, D(1, 2), 2, 4, out(16))
# ---- CSC (.) dense: (p, ncols, i, x, dense, nrows, ...)
for sfx, x, d in (("multiply_csc_by_dense_ignore_NAs_numeric", X2, D(1, 2, 3, 4)),
                  ("multiply_csc_by_dense_ignore_NAs_float32", X2, F(1, 2, 3, 4)),
                  ("multiply_csc_by_dense_ignore_NAs_integer", X2, I(1, 2, 3, 4)),
                  ("multiply_csc_by_dense_ignore_NAs_logical", X2, I(1, 0, 1, 0)),
                  ("logicaland_csc_by_dense_ignore_NAs", L2, I(1, 0, 1, 0))):
    call("mx_" + sfx, None, 2, J2, x, d, 2, out(16))
    call("mx_" + sfx, P2, -1, J2, x, d, 2, out(16))
    call("mx_" + sfx, P2, 2, J2, x, d, -1, out(16))
    call("mx_" + sfx, I(0), 0, E0, x, d, 2, out(16))
    call("mx_" + sfx, PNEG, 1, J2, x, d, 2, out(16))
for sfx, d in (("numeric", D(1, 2, 3, 4)), ("integer", I(1, 2, 3, 4)), ("logical", I(1, 0, 1, 0)), ("float32", F(1, 2, 3, 4))):
    fn = "mx_multiply_csc_by_dense_keep_NAs_" + sfx
    call(fn, P2, 2, J2, X2, d, 2, None, INFO)
    call(fn, P2, 2, J2, X2, d, 2, RES, None)
    call(fn, None, 2, J2, X2, d, 2, RES, INFO)
    call(fn, P2, -1, J2, X2, d, 2, RES, INFO)
    call(fn, P2, 2, J2, X2, d, -1, RES, INFO)
    call(fn, PBAD, 2, J2, X2, d, 2, RES, INFO)
    call(fn, PNEG, 1, J2, X2, d, 2, RES, INFO)
# ---- mx_multiply_csr_by_svec_begin(p, nrows, j, x, ii_base1, xx, nnz_v, ncols, length, keep_NAs, res, info)
fn = "mx_multiply_csr_by_svec_begin"
call(fn, P2, 2, J2, X2, I(1), D(2.0), 1, 2, 2, 0, None, INFO)
call(fn, None, 2, J2, X2, I(1), D(2.0), 1, 2, 2, 0, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), D(2.0), -1, 2, 2, 0, RES, INFO)
call(fn, PBAD, 2, J2, X2, I(1), D(2.0), 1, 2, 2, 0, RES, INFO)
call(fn, PNEG, 1, J2, X2, I(1), D(2.0), 1, 2, 1, 0, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), D(2.0), 1, 2, 0, 0, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), D(2.0), 1, 2, 3, 0, RES, INFO)
call(fn, I(0, 1, 2, 2), 3, J2, X2, I(1), D(2.0), 1, 2, 2, 0, RES, INFO)
call(fn, P2, 2, J2, X2, I(1, 2), D(2.0, 3.0), 2, 2, 1, 1, RES, INFO)
# ---- dense matrix * sparse vector
fn = "mx_dense_by_svec_route"                           # (nrows, ncols, length)
for a in ((-1, 2, 2), (2, -1, 2), (2, 2, -1), (2, 2, 0), (0, 2, 0), (2, 3, 6), (4, 3, 4), (4, 3, 2), (4, 3, 3), (4, 3, 8),
          (1, 1, 1), (0, 0, 5)):
    call(fn, *a)
X8 = D(1, 2, 3, 4, 5, 6, 7, 8)
for fn, tail, ok, other in (("mx_multiply_elemwise_dense_by_svec_begin", [RES, INFO], 4, 8),
                            ("mx_multiply_elemwise_dense_by_svec_dense", [out(72)], 8, 4)):
    # (X, kind, nrows, ncols, ii_base1, xx, nnz_v, length, keep_NAs, ...) on a 4 x 2 matrix
    call(fn, X8, 4, 4, 2, I(1), D(2.0), 1, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1), D(2.0), -1, ok, 0, *tail)
    call(fn, X8, 0, -4, 2, I(1), D(2.0), 1, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1), D(2.0), 1, 0, 0, *tail)
    call(fn, None, 0, 4, 2, I(1), D(2.0), 1, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, None, D(2.0), 1, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1), None, 1, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1, 2, 3), D(1, 2, 3), 3, 2, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1, 0), D(1, 2), 2, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1, 9), D(1, 2), 2, ok, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1), D(2.0), 1, other, 0, *tail)
    call(fn, X8, 0, 4, 2, I(1), D(2.0), 1, 2 if other == 4 else 3, 1, *tail)
call("mx_multiply_elemwise_dense_by_svec_begin", X8, 0, 4, 2, I(1), D(2.0), 1, 4, 0, None, INFO)
call("mx_multiply_elemwise_dense_by_svec_begin", X8, 0, 4, 2, I(1), D(2.0), 1, 4, 0, RES, None)
call("mx_multiply_elemwise_dense_by_svec_dense", None, 0, 0, 2, None, None, 0, 0, 0, out(72))    # no cells
call("mx_multiply_elemwise_dense_by_svec_dense", None, 1, 4, 0, I(1), D(2.0), 1, 3, 1, out(72))  # no cells, route D
call("mx_multiply_elemwise_dense_by_svec_dense", X8, 0, 4, 2, I(1), D(2.0), 1, 8, 0, None)
# ---- COO * dense matrix, values only: (X, nrows, ncols, ii, jj, xx, nnz, values_out)
for sfx, X, x in (("multiply_coo_by_dense_numeric", D(1, 2, 3, 4), X2), ("multiply_coo_by_dense_integer", I(1, 2, 3, 4), X2),
                  ("multiply_coo_by_dense_logical", I(1, 0, 1, 0), X2), ("multiply_coo_by_dense_float32", F(1, 2, 3, 4), X2),
                  ("logicaland_coo_by_dense_logical", I(1, 0, 1, 0), L2)):
    fn = "mx_" + sfx
    call(fn, X, -1, 2, J2, J2, x, 2, out(16))
    call(fn, X, 2, -1, J2, J2, x, 2, out(16))
    call(fn, X, 2, 2, J2, J2, x, -1, out(16))
    call(fn, X, 2, 2, J2, J2, x, 2**31, out(16))
    call(fn, X, 2, 2, None, None, None, 0, out(16))
    call(fn, X, 2, 2, None, J2, x, 2, out(16))
    call(fn, X, 2, 2, J2, None, x, 2, out(16))
    call(fn, X, 2, 2, J2, J2, None, 2, out(16))
    call(fn, X, 2, 2, J2, J2, x, 2, None)
    call(fn, X, 2, 2, I(0, 2), J2, x, 2, out(16))
    call(fn, X, 2, 2, J2, I(-1, 1), x, 2, out(16))
    call(fn, None, 2, 2, J2, J2, x, 2, out(16))
# ---- outer products, row vector x CSC
fn = "mx_matmul_colvec_by_scolvecascsr_begin"           # (colvec, dtype, dim, p, nrows, j, x, res, info)
call(fn, D(1, 2), F64, 2, P2, 2, J2, X2, None, INFO)
call(fn, D(1, 2), F64, 2, None, 2, J2, X2, RES, INFO)
call(fn, D(1, 2), F64, -1, P2, 2, J2, X2, RES, INFO)
call(fn, None, F64, 2, P2, 2, J2, X2, RES, INFO)
call(fn, D(1, 2), LGL, 2, P2, 2, J2, X2, RES, INFO)
call(fn, D(1, 2), F64, 2, PNEG, 1, J2, X2, RES, INFO)
call(fn, D(1, 2), F64, 2, I(-1, 1), 1, J2, X2, RES, INFO)
call(fn, D(1, 2), F64, INT_MAX, P2, 2, J2, X2, RES, INFO)
fn = "mx_matmul_spcolvec_by_scolvecascsr_begin"         # (Xp, nrows, Xj, Xx, y_base1, y_values, dtype, nnz_y, y_length, res, info)
call(fn, P2, 2, J2, X2, I(1), D(2.0), F64, 1, 3, RES, None)
call(fn, None, 2, J2, X2, I(1), D(2.0), F64, 1, 3, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), D(2.0), F64, 2**31, 3, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), D(2.0), F64, 1, -1, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), D(2.0), F32, 1, 3, RES, INFO)
call(fn, P2, 2, J2, X2, None, D(2.0), F64, 1, 3, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), None, I32, 1, 3, RES, INFO)
call(fn, PNEG, 1, J2, X2, I(1), D(2.0), F64, 1, 3, RES, INFO)
call(fn, P2, 2, J2, X2, I(1), None, NONE, INT_MAX, 3, RES, INFO)
fn = "mx_matmul_rowvec_by_csc"                          # (rowvec, len_rowvec, p, ncols, i, x, out)
call(fn, F(1, 2), 2, P2, -1, J2, X2, out(8))
call(fn, F(1, 2), -1, P2, 2, J2, X2, out(8))
call(fn, F(1, 2), 2, I(0), 0, E0, D(), out(8))
call(fn, F(1, 2), 2, None, 2, J2, X2, out(8))
call(fn, F(1, 2), 2, P2, 2, J2, X2, None)
call(fn, F(1, 2), 2, PNEG, 1, J2, X2, out(8))
# ---- CSR (op) dense vector: (p, j, x, nrows, dvec, dvec_len, ncols, [five flags, X_is_LHS,] ...)
fn = "mx_multiply_csr_by_dvec_no_NAs_numeric"
call(fn, P2, J2, X2, 2, D(1, 2), 2, 2, 0, 0, 0, 0, 0, 1, out(16))
call(fn, P2, J2, X2, -1, D(1, 2), 2, 2, 1, 0, 0, 0, 0, 1, out(16))
call(fn, P2, J2, X2, 2, D(1, 2), 2, -1, 0, 1, 0, 0, 0, 1, out(16))
call(fn, P2, J2, X2, 2, D(1, 2), -1, 2, 0, 0, 1, 0, 0, 1, out(16))
call(fn, I(0), E0, D(), 0, D(1, 2), 2, 2, 0, 0, 0, 1, 0, 1, out(16))
call(fn, None, J2, X2, 2, D(1, 2), 2, 2, 0, 0, 0, 0, 1, 0, out(16))
call(fn, PNEG, J2, X2, 1, D(1, 2), 2, 2, 1, 1, 1, 1, 1, 1, out(16))
fn = "mx_logicaland_csr_by_dvec_internal"
call(fn, P2, J2, L2, -1, I(1, 0), 2, 2, out(8))
call(fn, I(0), E0, E0, 0, I(1, 0), 2, 2, out(8))
call(fn, None, J2, L2, 2, I(1, 0), 2, 2, out(8))
call(fn, PNEG, J2, L2, 1, I(1, 0), 2, 2, out(8))
fn = "mx_multiply_csr_by_dvec_with_NAs_begin"           # (..., res, info)
call(fn, P2, J2, X2, 2, D(1, 2), 2, 2, 1, 0, 0, 0, 0, 1, None, INFO)
call(fn, None, J2, X2, 2, D(1, 2), 2, 2, 1, 0, 0, 0, 0, 1, RES, INFO)
call(fn, P2, J2, X2, 2, None, 2, 2, 1, 0, 0, 0, 0, 1, RES, INFO)
call(fn, P2, J2, X2, -1, D(1, 2), 2, 2, 1, 0, 0, 0, 0, 1, RES, INFO)
for flags in ((0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (1, 0, 0, 1, 0)):
    call(fn, P2, J2, X2, 2, D(1, 2), 2, 2, *flags, 0, RES, INFO)                     # X on the right
call(fn, P2, J2, X2, 2, D(1, 2), 2, 2, 0, 0, 0, 0, 0, 1, RES, INFO)
call(fn, P2, J2, X2, 2, D(1, 2), 2, 2, 0, 0, 0, 0, 0, 0, RES, INFO)
call(fn, PBAD, J2, X2, 2, D(1, 2), 2, 2, 1, 0, 0, 0, 0, 1, RES, INFO)
call(fn, PNEG, J2, X2, 1, D(1, 2), 2, 2, 0, 0, 0, 0, 1, 0, RES, INFO)
call(fn, P2, J2, X2, 2, D(1, 2), 0, 2, 1, 0, 0, 0, 0, 1, RES, INFO)
call(fn, P2, J2, X2, 2, D(1, 2, 3, 4, 5), 5, 2, 1, 0, 0, 0, 0, 1, RES, INFO)
# ---- cbind / rbind
fn = "mx_cbind_csr_begin"                               # (Xp, nX, Xj, Xx, nvX, Yp, nY, Yj, Yx, nvY, dtype, res, info)
call(fn, P2, 2, J2, X2, 2, P2, 2, J2, X2, 2, F64, None, INFO)
call(fn, P2, -1, J2, X2, 2, P2, 2, J2, X2, 2, F64, RES, INFO)
call(fn, P2, 2, J2, X2, 2, P2, -1, J2, X2, 2, F64, RES, INFO)
call(fn, None, 2, J2, X2, 2, P2, 2, J2, X2, 2, F64, RES, INFO)
call(fn, PNEG, 1, J2, X2, 2, P2, 2, J2, X2, 2, NONE, RES, INFO)
fn = "mx_concat_csr_batch_begin"                        # (objects, n_inputs, out_kind, res, info)
ONE = ["rbind", [[0, P2, J2, X2, 2, 2]]]
call(fn, ONE, 1, 0, RES, None)
call(fn, ONE, -1, 0, RES, INFO)
call(fn, ONE, 1, 3, RES, INFO)
call(fn, ["rbind", [[0, P2, J2, X2, 2, 2], [7, None, J2, X2, 0, 2]]], 2, 0, RES, INFO)
call(fn, ["rbind", [[-1, P2, J2, X2, 2, 2]]], 1, 1, RES, INFO)
call(fn, ["rbind", [[3, None, J2, X2, 0, INT_MAX], [3, None, J2, X2, 0, 1]]], 2, 0, RES, INFO)
call(fn, ["rbind", [[0, P2, J2, X2, INT_MAX - 1, 2], [6, None, J2, None, 0, 2]]], 2, 2, RES, INFO)
# ---- transpose, COO conversions
fn = "mx_csr_transpose_begin"                           # (p, nrows, ncols, j, x, dtype, n_values, res, info)
call(fn, P2, 2, 2, J2, X2, F64, 2, None, INFO)
call(fn, None, 2, 2, J2, X2, F64, 2, RES, INFO)
call(fn, P2, -1, 2, J2, X2, F64, 2, RES, INFO)
call(fn, P2, 2, -1, J2, X2, F64, 2, RES, INFO)
call(fn, P2, 2, 2, J2, X2, I32, 2, RES, INFO)
call(fn, PBAD, 2, 2, J2, X2, F64, 2, RES, INFO)
call(fn, PNEG, 1, 2, J2, X2, F64, 2, RES, INFO)
call(fn, P2, 2, 2, J2, X2, F64, 1, RES, INFO)
fn = "mx_coo_to_csr_begin"                              # (rows, cols, values, dtype, n_entries, nrows, ncols, res, info)
call(fn, J2, J2, X2, F64, 2, 2, 2, RES, None)
call(fn, J2, J2, X2, F64, 2, -1, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2, 2, -1, RES, INFO)
call(fn, J2, J2, X2, F64, -1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2**31, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F32, 2, 2, 2, RES, INFO)
fn = "mx_csr_to_coo"                                    # (p, nrows, out_rows)
call(fn, None, 2, out(8))
call(fn, P2, -1, out(8))
call(fn, PBAD, 2, out(8))
call(fn, PNEG, 1, out(8))
call(fn, PE, 2, out(8))
call(fn, P2, 2, None)
fn = "mx_multiply_csr_by_coo_begin"     # (logical, Xp, Xj, Xx, Yr, Yc, Yv, nnz_Y, max_row_X, max_col_X, res, info)
call(fn, 0, P2, J2, X2, J2, J2, X2, 2, 2, 2, None, INFO)
call(fn, 0, None, J2, X2, J2, J2, X2, 2, 2, 2, RES, INFO)
call(fn, 0, P2, J2, X2, J2, J2, X2, 2, -1, 2, RES, INFO)
call(fn, 0, P2, J2, X2, J2, J2, X2, 2, 2, -1, RES, INFO)
call(fn, 0, P2, J2, X2, J2, J2, X2, -1, 2, 2, RES, INFO)
call(fn, 1, P2, J2, L2, J2, J2, L2, 2**31, 2, 2, RES, INFO)
call(fn, 0, PNEG, J2, X2, J2, J2, X2, 2, 1, 2, RES, INFO)
# ---- COO (op) dense vector: (ii, jj, xx, nnz, dvec, dvec_len, nrows, ncols, ...)
fn = "mx_multiply_coo_by_dense_ignore_NAs_numeric"
call(fn, J2, J2, X2, 2, D(1, 2), 2, 2, 2, 0, 0, 0, 0, 0, 1, out(16))
call(fn, J2, J2, X2, 2, D(1, 2), 2, -1, 2, 1, 0, 0, 0, 0, 1, out(16))
call(fn, J2, J2, X2, -1, D(1, 2), 2, 2, 2, 0, 1, 0, 0, 0, 1, out(16))
call(fn, J2, J2, X2, 2, D(1, 2), -1, 2, 2, 0, 0, 1, 0, 0, 1, out(16))
call(fn, None, None, None, 0, D(1, 2), 2, 2, 2, 0, 0, 0, 1, 0, 1, out(16))
call(fn, J2, J2, X2, 2, None, 0, 2, 2, 0, 0, 0, 0, 1, 0, out(16))
fn = "mx_multiply_coo_by_dense_ignore_NAs_logical"
call(fn, J2, J2, L2, 2, I(1, 0), 2, 2, -1, out(8))
call(fn, None, None, None, 0, I(1, 0), 2, 2, 2, out(8))
call(fn, J2, J2, L2, 2, None, 0, 2, 2, out(8))
# ---- X[i, j] of a COO
fn = "mx_slice_coo_arbitrary_begin"     # (ii, jj, xx, dtype, nnz, rows_base1, n_rows, cols_base1, n_cols, all_i, all_j,
#                                          i_is_seq, j_is_seq, i_is_rev_seq, j_is_rev_seq, nrows, ncols, res, info)
T = (I(1, 2), 2, I(2, 1), 2)
call(fn, J2, J2, X2, F64, 2, *T, 0, 0, 1, 0, 0, 1, 2, 2, None, INFO)
call(fn, J2, J2, X2, F64, 2, *T, 0, 0, 1, 0, 0, 1, -1, 2, RES, INFO)
call(fn, J2, J2, X2, F64, -1, *T, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2, I(1, 2), -1, I(2, 1), 2, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2**31, *T, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, I32, 2, *T, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, None, J2, X2, F64, 2, *T, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, None, LGL, 2, *T, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2, None, 2, I(2, 1), 2, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2, I(1, 2), 2, None, 2, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)
call(fn, J2, J2, X2, F64, 2, I(1, 3), 2, I(2, 1), 2, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)      # row seq outside
call(fn, J2, J2, X2, F64, 2, I(2, 1), 2, I(2, 1), 2, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)      # not ascending
call(fn, J2, J2, X2, F64, 2, I(1, 2), 2, I(2, 1), 2, 0, 0, 0, 0, 1, 1, 2, 2, RES, INFO)      # not descending
call(fn, J2, J2, X2, F64, 2, I(2, 0, 1), 3, I(2, 1), 2, 0, 0, 0, 0, 0, 1, 2, 2, RES, INFO)   # row map outside
call(fn, J2, J2, X2, F64, 2, I(1, 2), 2, I(0, 1), 2, 0, 0, 1, 0, 0, 1, 2, 2, RES, INFO)      # column seq outside
call(fn, J2, J2, X2, F64, 2, I(1, 2), 2, I(1, 2), 2, 1, 0, 0, 0, 0, 1, 2, 2, RES, INFO)      # column not descending
call(fn, J2, J2, X2, F64, 2, I(1, 2), 2, I(1, 3, 1), 3, 1, 0, 0, 0, 0, 0, 2, 2, RES, INFO)   # column map outside
fn = "mx_slice_coo_single"                              # (ii, jj, xx, dtype, nnz, i, j, found, value_out)
call(fn, J2, J2, X2, F64, 2, 0, 0, None, out(8))
call(fn, J2, J2, X2, F64, -1, 0, 0, out(4), out(8))
call(fn, J2, J2, X2, F32, 2, 0, 0, out(4), out(8))
call(fn, None, None, None, F64, 0, 0, 0, out(4), out(8))
call(fn, None, J2, X2, F64, 2, 0, 0, out(4), out(8))
call(fn, J2, J2, None, LGL, 2, 0, 0, out(4), out(8))
# ---- the compaction
for sfx, x in (("csr_numeric", X2), ("csr_logical", L2)):
    fn = "mx_remove_zero_valued_" + sfx                 # (p, j, x, nrows, remove_NAs, res, info)
    call(fn, P2, J2, x, 2, 0, None, INFO)
    call(fn, P2, J2, x, 2, 0, RES, None)
    call(fn, P2, J2, x, -1, 0, RES, INFO)
    call(fn, P2, J2, x, INT_MAX, 0, RES, INFO)
    call(fn, None, J2, x, 2, 1, RES, INFO)
    call(fn, PBAD, J2, x, 2, 1, RES, INFO)
    call(fn, PNEG, J2, x, 1, 1, RES, INFO)
    call(fn, P2, None, x, 2, 0, RES, INFO)
    call(fn, P2, J2, None, 2, 0, RES, INFO)
for sfx, x in (("coo_numeric", X2), ("coo_logical", L2)):
    fn = "mx_remove_zero_valued_" + sfx                 # (ii, jj, xx, nnz, remove_NAs, res, info)
    call(fn, J2, J2, x, 2, 0, None, INFO)
    call(fn, J2, J2, x, -1, 0, RES, INFO)
    call(fn, J2, J2, x, 2**31, 0, RES, INFO)
    call(fn, None, J2, x, 2, 1, RES, INFO)
    call(fn, J2, None, x, 2, 1, RES, INFO)
    call(fn, J2, J2, None, 2, 1, RES, INFO)
for sfx, x in (("svec_numeric", X2), ("svec_integer", L2), ("svec_logical", L2)):
    fn = "mx_remove_zero_valued_" + sfx                 # (ii, xx, nnz, remove_NAs, res, info)
    call(fn, J2, x, 2, 0, RES, None)
    call(fn, J2, x, -1, 0, RES, INFO)
    call(fn, J2, x, 2**31, 1, RES, INFO)
    call(fn, None, x, 2, 1, RES, INFO)
    call(fn, J2, None, 2, 1, RES, INFO)
fn = "mx_filter_sparse_begin"           # (layout, p, nrows, idx0, idx1, x, dtype, nnz, mask, res, info)
call(fn, 0, P2, 2, J2, None, X2, F64, 2, L2, None, INFO)
call(fn, -1, P2, 2, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 3, P2, 2, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 1, None, -1, J2, J2, X2, F64, 2, L2, RES, INFO)
call(fn, 2, None, INT_MAX, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 0, P2, 2, J2, None, X2, F32, 2, L2, RES, INFO)
call(fn, 1, None, 0, J2, J2, X2, NONE, 2, L2, RES, INFO)
call(fn, 0, None, 2, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 0, PBAD, 2, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 0, PNEG, 1, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 1, None, 0, J2, J2, X2, F64, -1, L2, RES, INFO)
call(fn, 2, None, 0, J2, None, X2, I32, 2**31, L2, RES, INFO)
call(fn, 0, P2, 2, None, None, X2, F64, 2, L2, RES, INFO)
call(fn, 1, None, 0, J2, None, X2, F64, 2, L2, RES, INFO)
call(fn, 2, None, 0, J2, None, None, LGL, 2, L2, RES, INFO)
call(fn, 2, None, 0, J2, None, L2, LGL, 2, None, RES, INFO)
fn = "mx_rebuild_indptr_after_filter"                   # (p, indptr_len, filter, out_indptr)
call(fn, P2, -1, L2, out(16))
call(fn, P2, 2**31, L2, out(16))
call(fn, None, 0, None, out(16))
call(fn, None, 3, L2, out(16))
call(fn, P2, 3, L2, None)
call(fn, PBAD, 3, L2, out(16))
call(fn, PNEG, 2, L2, out(16))
call(fn, P2, 3, None, out(16))
# ---- check_sparse_matrix
call("mx_check_valid_csr_matrix", P2, 3, J2, 2, 2, 2, None)       # (p, indptr_len, j, nnz, nrows, ncols, err)
call("mx_check_valid_csr_matrix", P2, -1, J2, 2, 2, 2, out(8))
call("mx_check_valid_csr_matrix", P2, 3, J2, -1, 2, 2, out(8))
call("mx_check_valid_csr_matrix", None, 3, J2, 2, 2, 2, out(8))
call("mx_check_valid_csr_matrix", P2, 3, None, 2, 2, 2, out(8))
call("mx_check_valid_coo_matrix", J2, J2, 2, 2, 2, None)          # (ii, jj, nnz, nrows, ncols, err)
call("mx_check_valid_coo_matrix", J2, J2, -1, 2, 2, out(8))
call("mx_check_valid_coo_matrix", None, J2, 2, 2, 2, out(8))
call("mx_check_valid_coo_matrix", J2, None, 2, 2, 2, out(8))
call("mx_check_valid_svec", J2, 2, 2, None)                       # (ii, nnz, nrows, err)
call("mx_check_valid_svec", J2, -1, 2, out(8))
call("mx_check_valid_svec", None, 2, 2, out(8))
# ---- results
call("mx_result_finish", None, out(8), out(8), out(8))
call("mx_result_discard", None)
# ---- index-vector classification, sorting
for fn, asc, desc in (("mx_check_is_seq", I(3, 4, 5), I(5, 4, 3)), ("mx_check_is_rev_seq", I(5, 4, 3), I(3, 4, 5))):
    call(fn, asc, 3, None)                              # (indices, n, result)
    call(fn, None, 0, out(4))
    call(fn, I(7), 1, out(4))
    call(fn, desc, 3, out(4))
fn = "mx_check_indices_are_sorted"                      # (p, j, nrows, result)
call(fn, P2, J2, 2, None)
call(fn, P2, J2, 0, out(4))
call(fn, P2, J2, -1, out(4))
call(fn, None, J2, 2, out(4))
call(fn, PNEG, J2, 1, out(4))
fn = "mx_sort_sparse_indices"                           # (p, j, x, dtype, nrows)
call(fn, P2, out(8), out(16), F64, 0)
call(fn, P2, out(8), out(16), F64, -1)
call(fn, None, out(8), out(16), F64, 2)
call(fn, PNEG, out(8), None, NONE, 1)
fn = "mx_sort_vector_indices"                           # (ii, xx, n, dtype)
call(fn, out(8), out(16), -1, F64)
call(fn, out(8), out(16), 2**31, F64)
call(fn, out(8), out(16), 1, F64)
call(fn, None, None, 0, NONE)
call(fn, None, out(16), 2, F64)
call(fn, out(8), None, 2, F64)
call(fn, out(8), out(16), 2, 5)
fn = "mx_sort_coo_indices"                              # (ii, jj, xx, nnz, dtype)
call(fn, out(8), out(8), out(16), -1, F64)
call(fn, out(8), out(8), out(16), 2**31, F64)
call(fn, out(8), out(8), out(16), 2, I32)
call(fn, None, None, None, 0, NONE)
call(fn, None, out(8), out(16), 2, F64)
call(fn, out(8), None, out(16), 2, LGL)
call(fn, out(8), out(8), None, 2, F64)


def main(only):
    record = []
    if only:
        with open(PATH) as f:
            record = [e for e in json.load(f) if e["call"][0] not in only]
    for fn, args in CALLS:
        if only and fn not in only:
            continue
        record.append({"call": [fn, args], "result": run_call(fn, args)})
    record.sort(key=lambda e: e["call"][0])             # stable: a function's calls keep their order
    with open(PATH, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in record) + "\n]\n")
    print(f"{PATH}: {len({e['call'][0] for e in record})} functions, {len(record)} calls, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
