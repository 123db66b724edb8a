#!/usr/bin/env python3
"""Generates tests/golden/export_result_shapes.json: what every *_begin export of the C-ABI reports in its
mx_result_info and hands out through mx_result_finish, at the small shapes where the result-sizing branches differ
(at most 6 rows, 8 columns, 12 entries): a non-empty result, an empty one, a call without values where the export
admits one, and the aliasing paths (identical-structure `+` and `-` of an object with itself; no new cell in the
flat regime of multiply_csr_by_dvec_with_NAs; a zero rule that removes nothing in the compaction; the CSC (.) dense
product whose structure does not change).

The record was taken ONCE, on an MI355X, from the library built at the commit before the export layer got its typed
device arrays and mx_result its shaping members (csrc/api.hip), and is what tests/test_gpu_export_result_shapes.py
holds every later build to, bit for bit.  Do not regenerate it from the code under test; a new export is recorded
when it is added and left alone afterwards (run with its case names to add only those).
Run from the repo root, on a machine with a device:  python tests/golden/make_export_result_shapes.py [case ...]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from export_calls import run_call  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "export_result_shapes.json")
F64, F32, I32, LGL, NONE = 0, 1, 2, 3, 4
NA_REAL = 0x7FF00000000007A2
NA_INT = -2**31
R, NFO = "res", "info"


def I(*v):
    return ["i32", [int(k) for k in v]]


def D(*v):
    """doubles as bit patterns; an int >= 2**52 is taken as a bit pattern already (NA_REAL)"""
    return ["u64", [k if isinstance(k, int) and k >= 2**52 else int(np.float64(k).view(np.uint64)) for k in v]]


def F(*v):
    return ["u32", [int(np.float32(k).view(np.uint32)) for k in v]]


NAN = float("nan")
# A: 4 x 6, rows {1,4} {} {0,2,5} {3}
AP, AJ, AX = I(0, 2, 2, 5, 6), I(1, 4, 0, 2, 5, 3), D(1.5, -2.0, 3.0, NA_REAL, 0.5, 4.0)
AL = I(1, 0, NA_INT, 1, 1, 0)                                    # A's entries as R logicals
# B: 4 x 6, rows {1} {0,2} {} {3}
BP, BJ, BX = I(0, 1, 3, 3, 4), I(1, 0, 2, 3), D(2.0, 7.0, -1.0, 0.25)
BL = I(1, 1, 0, NA_INT)
# Z: 4 x 6 whose pattern misses A's: rows {0} {1} {1} {}
ZP, ZJ, ZX = I(0, 1, 2, 3, 3), I(0, 1, 1), D(1.0, 2.0, 3.0)
EP = I(0, 0, 0, 0, 0)                                            # 4 empty rows
E0 = I()
# A as a COO, shuffled, with one repeated cell
CI, CJ, CX = I(2, 0, 3, 2, 0, 2, 2), I(5, 1, 3, 0, 4, 2, 5), D(0.5, 1.5, 4.0, 3.0, -2.0, NA_REAL, 1.0)
CL = I(1, 1, 0, NA_INT, 1, 1, 0)

CASES = {}


def case(name, fn, *args):
    assert name not in CASES
    CASES[name] = [fn, list(args)]


# ---- mx_csr_elemwise_begin(op, nrows, p1, p2, j1, j2, x1, x2, nnz1, nnz2)
case("elemwise_add", "mx_csr_elemwise_begin", 0, 4, AP, BP, AJ, BJ, AX, BX, 6, 4, R, NFO)
case("elemwise_mul_empty", "mx_csr_elemwise_begin", 2, 4, AP, ZP, AJ, ZJ, AX, ZX, 6, 3, R, NFO)
case("elemwise_or_logical", "mx_csr_elemwise_begin", 3, 4, AP, BP, AJ, BJ, AL, BL, 6, 4, R, NFO)
case("elemwise_and_empty", "mx_csr_elemwise_begin", 5, 4, AP, ZP, AJ, ZJ, AL, I(1, 1, 1), 6, 3, R, NFO)
case("elemwise_add_alias", "mx_csr_elemwise_begin", 0, 4, AP, ["same", 2], AJ, ["same", 4], AX,
     D(1.0, 2.0, 3.0, 4.0, 5.0, 6.0), 6, 6, R, NFO)
case("elemwise_sub_self", "mx_csr_elemwise_begin", 1, 4, AP, ["same", 2], AJ, ["same", 4], AX, ["same", 6], 6, 6, R,
     NFO)
case("elemwise_xor_alias", "mx_csr_elemwise_begin", 4, 4, AP, ["same", 2], AJ, ["same", 4], AL, I(1, 1, 0, 0, NA_INT, 0),
     6, 6, R, NFO)
# ---- mx_copy_csr_rows_begin(p, nrows, j, x, dtype, n_values, rows, n_take)
case("gather", "mx_copy_csr_rows_begin", AP, 4, AJ, AX, F64, 6, I(2, 0, 2), 3, R, NFO)
case("gather_empty", "mx_copy_csr_rows_begin", AP, 4, AJ, AX, F64, 6, I(1, 1), 2, R, NFO)
case("gather_logical", "mx_copy_csr_rows_begin", AP, 4, AJ, AL, LGL, 6, I(3, 2), 2, R, NFO)
case("gather_none", "mx_copy_csr_rows_begin", AP, 4, AJ, None, NONE, 0, I(2, 0, 2), 3, R, NFO)
case("gather_no_values", "mx_copy_csr_rows_begin", AP, 4, AJ, None, F64, 0, I(0, 3), 2, R, NFO)
case("gather_none_empty", "mx_copy_csr_rows_begin", AP, 4, AJ, None, NONE, 0, I(1), 1, R, NFO)
# ---- mx_copy_csr_rows_col_seq_begin(p, nrows, j, x, dtype, n_values, rows, n_take, cols, n_cols, index1)
case("colseq", "mx_copy_csr_rows_col_seq_begin", AP, 4, AJ, AX, F64, 6, I(2, 0, 3), 3, I(2, 3, 4, 5), 4, 0, R, NFO)
case("colseq_index1", "mx_copy_csr_rows_col_seq_begin", AP, 4, AJ, AX, F64, 6, I(2, 0, 3), 3, I(3, 4, 5, 6), 4, 1, R, NFO)
case("colseq_empty", "mx_copy_csr_rows_col_seq_begin", AP, 4, AJ, AX, F64, 6, I(1, 3), 2, I(0, 1), 2, 0, R, NFO)
case("colseq_logical", "mx_copy_csr_rows_col_seq_begin", AP, 4, AJ, AL, LGL, 6, I(2, 0), 2, I(0, 1, 2), 3, 0, R, NFO)
case("colseq_none", "mx_copy_csr_rows_col_seq_begin", AP, 4, AJ, None, NONE, 0, I(2, 0), 2, I(0, 1, 2), 3, 0, R, NFO)
case("colseq_none_empty", "mx_copy_csr_rows_col_seq_begin", AP, 4, AJ, None, NONE, 0, I(1), 1, I(0, 1, 2), 3, 0, R, NFO)
# ---- mx_copy_csr_arbitrary_begin(p, nrows, j, x, dtype, n_values, rows, n_take, cols, n_cols)
case("arbitrary_unsorted", "mx_copy_csr_arbitrary_begin", AP, 4, AJ, AX, F64, 6, I(2, 0, 2), 3, I(5, 2, 2, 0, 1), 5, R, NFO)
case("arbitrary_sorted", "mx_copy_csr_arbitrary_begin", AP, 4, AJ, AX, F64, 6, I(3, 2), 2, I(0, 2, 3, 5), 4, R, NFO)
case("arbitrary_empty", "mx_copy_csr_arbitrary_begin", AP, 4, AJ, AX, F64, 6, I(1, 3), 2, I(2, 0), 2, R, NFO)
case("arbitrary_logical", "mx_copy_csr_arbitrary_begin", AP, 4, AJ, AL, LGL, 6, I(2, 0), 2, I(5, 1, 0), 3, R, NFO)
case("arbitrary_none", "mx_copy_csr_arbitrary_begin", AP, 4, AJ, None, NONE, 0, I(2, 0), 2, I(5, 1, 0), 3, R, NFO)
case("arbitrary_no_values_empty", "mx_copy_csr_arbitrary_begin", AP, 4, AJ, None, F64, 0, I(1), 1, I(0), 1, R, NFO)
# ---- mx_reverse_rows_begin(p, nrows, j, x, dtype, n_values)
case("reverse_rows", "mx_reverse_rows_begin", AP, 4, AJ, AX, F64, 6, R, NFO)
case("reverse_rows_empty", "mx_reverse_rows_begin", EP, 4, E0, D(), F64, 0, R, NFO)
case("reverse_rows_logical", "mx_reverse_rows_begin", AP, 4, AJ, AL, LGL, 6, R, NFO)
case("reverse_rows_none", "mx_reverse_rows_begin", AP, 4, AJ, None, NONE, 0, R, NFO)
# ---- mx_multiply_csc_by_dense_keep_NAs_*(p, ncols, i, x, dense, nrows): A read as a 6 x 4 CSC
DN = [1.0] * 24
case("csc_keep_same_structure", "mx_multiply_csc_by_dense_keep_NAs_numeric", AP, 4, AJ, AX, D(*range(1, 25)), 6, R, NFO)
DN[1 + 6 * 0], DN[3 + 6 * 1] = NAN, NA_REAL                      # a stored cell and one outside the pattern
case("csc_keep_new_cells", "mx_multiply_csc_by_dense_keep_NAs_numeric", AP, 4, AJ, AX, D(*DN), 6, R, NFO)
case("csc_keep_empty", "mx_multiply_csc_by_dense_keep_NAs_numeric", EP, 4, E0, D(), D(*range(24)), 6, R, NFO)
case("csc_keep_integer", "mx_multiply_csc_by_dense_keep_NAs_integer", AP, 4, AJ, AX,
     I(*[NA_INT if k in (0, 9) else k for k in range(24)]), 6, R, NFO)
case("csc_keep_logical_same", "mx_multiply_csc_by_dense_keep_NAs_logical", AP, 4, AJ, AX, I(*[k % 2 for k in range(24)]),
     6, R, NFO)
case("csc_keep_float32", "mx_multiply_csc_by_dense_keep_NAs_float32", AP, 4, AJ, AX,
     F(*[NAN if k == 7 else 0.5 * k for k in range(24)]), 6, R, NFO)
# ---- mx_multiply_csr_by_svec_begin(p, nrows, j, x, ii_base1, xx, nnz_v, ncols, length, keep_NAs)
case("csr_by_svec", "mx_multiply_csr_by_svec_begin", AP, 4, AJ, AX, I(1), D(3.0), 1, 6, 2, 0, R, NFO)
case("csr_by_svec_empty", "mx_multiply_csr_by_svec_begin", AP, 4, AJ, AX, I(2), D(3.0), 1, 6, 4, 0, R, NFO)
case("csr_by_svec_nothing_stored", "mx_multiply_csr_by_svec_begin", AP, 4, AJ, AX, None, None, 0, 6, 4, 0, R, NFO)
case("csr_by_svec_pattern", "mx_multiply_csr_by_svec_begin", AP, 4, AJ, AX, I(1, 3), None, 2, 6, 4, 0, R, NFO)
case("csr_by_svec_keep_na", "mx_multiply_csr_by_svec_begin", AP, 4, AJ, AX, I(1, 2), D(NAN, 2.0), 2, 6, 2, 1, R, NFO)
# ---- mx_multiply_elemwise_dense_by_svec_begin(X, kind, nrows, ncols, ii_base1, xx, nnz_v, length, keep_NAs)
case("dense_by_svec_b", "mx_multiply_elemwise_dense_by_svec_begin", D(*range(1, 9)), 0, 4, 2, I(2, 4), D(2.0, 3.0), 2, 4,
     0, R, NFO)
case("dense_by_svec_c", "mx_multiply_elemwise_dense_by_svec_begin", D(*range(1, 9)), 0, 4, 2, I(2), D(0.0), 1, 2, 0, R, NFO)
case("dense_by_svec_empty", "mx_multiply_elemwise_dense_by_svec_begin", D(*range(1, 9)), 0, 4, 2, None, None, 0, 4, 0, R,
     NFO)
case("dense_by_svec_integer_keep_na", "mx_multiply_elemwise_dense_by_svec_begin", I(1, NA_INT, 3, 4, 5, 6, NA_INT, 8), 2,
     4, 2, I(1), D(2.0), 1, 4, 1, R, NFO)
# ---- mx_matmul_colvec_by_scolvecascsr_begin(colvec, dtype, dim, p, nrows, j, x)
case("outer_dense", "mx_matmul_colvec_by_scolvecascsr_begin", D(1.0, -2.0, 0.0), F64, 3, I(0, 1, 1, 2), 3, I(0, 0),
     D(2.0, 5.0), R, NFO)
case("outer_dense_empty", "mx_matmul_colvec_by_scolvecascsr_begin", D(1.0, -2.0, 0.0), F64, 3, I(0, 0, 0, 0), 3, E0, D(), R,
     NFO)
case("outer_dense_no_dim", "mx_matmul_colvec_by_scolvecascsr_begin", None, F64, 0, I(0, 1, 1, 2), 3, I(0, 0), D(2.0, 5.0),
     R, NFO)
case("outer_dense_float32", "mx_matmul_colvec_by_scolvecascsr_begin", F(1.0, -2.0, 0.5), F32, 3, I(0, 1, 1, 2), 3, I(0, 0),
     D(2.0, 5.0), R, NFO)
# ---- mx_matmul_spcolvec_by_scolvecascsr_begin(Xp, nrows, Xj, Xx, y_base1, y_values, dtype, nnz_y, y_length)
case("outer_svec", "mx_matmul_spcolvec_by_scolvecascsr_begin", I(0, 1, 1, 2), 3, I(0, 0), D(2.0, 5.0), I(2, 5), D(3.0, NAN),
     F64, 2, 6, R, NFO)
case("outer_svec_empty", "mx_matmul_spcolvec_by_scolvecascsr_begin", I(0, 1, 1, 2), 3, I(0, 0), D(2.0, 5.0), None, None, F64,
     0, 6, R, NFO)
case("outer_svec_empty_rows", "mx_matmul_spcolvec_by_scolvecascsr_begin", I(0, 0, 0, 0), 3, E0, D(), I(2, 5), D(3.0, 1.0),
     F64, 2, 6, R, NFO)
case("outer_svec_none", "mx_matmul_spcolvec_by_scolvecascsr_begin", I(0, 1, 1, 2), 3, I(0, 0), D(2.0, 5.0), I(1, 6), None,
     NONE, 2, 6, R, NFO)
case("outer_svec_integer", "mx_matmul_spcolvec_by_scolvecascsr_begin", I(0, 1, 1, 2), 3, I(0, 0), D(2.0, 5.0), I(3, 4),
     I(NA_INT, 7), I32, 2, 6, R, NFO)
# ---- mx_multiply_csr_by_dvec_with_NAs_begin(p, j, x, nrows, dvec, dvec_len, ncols, mul, pow, div, rest, intdiv, lhs)
case("dvec_na_rows", "mx_multiply_csr_by_dvec_with_NAs_begin", AP, AJ, AX, 4, D(2.0, NAN), 2, 6, 1, 0, 0, 0, 0, 1, R, NFO)
case("dvec_na_rows_divide", "mx_multiply_csr_by_dvec_with_NAs_begin", AP, AJ, AX, 4, D(2.0, 0.0, 1.0, 4.0), 4, 6, 0, 0, 1, 0,
     0, 1, R, NFO)
case("dvec_na_rows_empty", "mx_multiply_csr_by_dvec_with_NAs_begin", EP, E0, D(), 4, D(1.0, 2.0), 2, 6, 1, 0, 0, 0, 0, 1, R,
     NFO)
case("dvec_na_flat_new_cells", "mx_multiply_csr_by_dvec_with_NAs_begin", AP, AJ, AX, 4, D(1.0, NA_REAL, 2.0, 3.0, 4.0, 5.0,
     6.0, 7.0, 8.0), 9, 6, 1, 0, 0, 0, 0, 1, R, NFO)
case("dvec_na_flat_power", "mx_multiply_csr_by_dvec_with_NAs_begin", AP, AJ, AX, 4, D(1.0, 2.0, 0.0, 3.0, -1.0, 5.0, 6.0,
     7.0, 8.0), 9, 6, 0, 1, 0, 0, 0, 1, R, NFO)
case("dvec_na_flat_alias", "mx_multiply_csr_by_dvec_with_NAs_begin", AP, AJ, AX, 4, D(1.0, 2.0, 3.0), 3, 6, 1, 0, 0, 0, 0, 1,
     R, NFO)
case("dvec_na_flat_alias_rhs", "mx_multiply_csr_by_dvec_with_NAs_begin", AP, AJ, AX, 4, D(1.0, 2.0, 3.0), 3, 6, 0, 0, 0, 0, 1,
     0, R, NFO)
case("dvec_na_flat_alias_empty", "mx_multiply_csr_by_dvec_with_NAs_begin", EP, E0, D(), 4, D(1.0, 2.0, 3.0), 3, 6, 1, 0, 0,
     0, 0, 1, R, NFO)
# ---- mx_cbind_csr_begin(Xp, nX, Xj, Xx, nvX, Yp, nY, Yj, Yx, nvY, dtype)
YP3, YJ3, YX3 = I(0, 1, 3, 3), I(7, 6, 8), D(9.0, 8.0, 7.0)
case("cbind", "mx_cbind_csr_begin", AP, 4, AJ, AX, 6, YP3, 3, YJ3, YX3, 3, F64, R, NFO)
case("cbind_empty", "mx_cbind_csr_begin", EP, 4, E0, D(), 0, I(0, 0, 0), 2, E0, D(), 0, F64, R, NFO)
case("cbind_logical", "mx_cbind_csr_begin", AP, 4, AJ, AL, 6, YP3, 3, YJ3, I(1, NA_INT, 0), 3, LGL, R, NFO)
case("cbind_none", "mx_cbind_csr_begin", AP, 4, AJ, None, 0, YP3, 3, YJ3, None, 0, NONE, R, NFO)
case("cbind_none_empty", "mx_cbind_csr_begin", EP, 4, E0, None, 0, I(0, 0, 0), 2, E0, None, 0, NONE, R, NFO)
# ---- mx_concat_csr_batch_begin(objects, n_inputs, out_kind)
case("rbind", "mx_concat_csr_batch_begin", ["rbind", [[0, AP, AJ, AX, 4, 6], [3, None, I(2, 6), D(1.0, NAN), 0, 2]]], 2, 0,
     R, NFO)
case("rbind_mixed", "mx_concat_csr_batch_begin", ["rbind", [[6, None, I(1), None, 0, 1], [1, BP, BJ, BL, 4, 4],
     [4, None, I(3, 5), I(NA_INT, 7), 0, 2]]], 3, 0, R, NFO)
case("rbind_empty", "mx_concat_csr_batch_begin", ["rbind", [[0, EP, E0, D(), 4, 0], [3, None, E0, D(), 0, 0]]], 2, 0, R, NFO)
case("rbind_no_inputs", "mx_concat_csr_batch_begin", None, 0, 0, R, NFO)
case("rbind_logical", "mx_concat_csr_batch_begin", ["rbind", [[1, BP, BJ, BL, 4, 4], [4, None, I(3), I(NA_INT), 0, 1],
     [3, None, I(2), D(0.0), 0, 1]]], 3, 1, R, NFO)
case("rbind_pattern", "mx_concat_csr_batch_begin", ["rbind", [[2, AP, AJ, None, 4, 6], [5, None, I(2, 4), I(1, 0), 0, 2]]],
     2, 2, R, NFO)
# ---- mx_csr_transpose_begin(p, nrows, ncols, j, x, dtype, n_values)
case("transpose", "mx_csr_transpose_begin", AP, 4, 6, AJ, AX, F64, 6, R, NFO)
case("transpose_merging", "mx_csr_transpose_begin", I(0, 3, 3), 2, 8, I(7, 2, 7), D(1.0, 2.0, 4.0), F64, 3, R, NFO)
case("transpose_empty", "mx_csr_transpose_begin", EP, 4, 6, E0, D(), F64, 0, R, NFO)
case("transpose_logical", "mx_csr_transpose_begin", AP, 4, 6, AJ, AL, LGL, 6, R, NFO)
case("transpose_none", "mx_csr_transpose_begin", AP, 4, 6, AJ, None, NONE, 0, R, NFO)
case("transpose_no_values", "mx_csr_transpose_begin", AP, 4, 6, AJ, None, F64, 0, R, NFO)
# ---- mx_coo_to_csr_begin(rows, cols, values, dtype, n_entries, nrows, ncols)
case("coo_to_csr", "mx_coo_to_csr_begin", CI, CJ, CX, F64, 7, 4, 6, R, NFO)
case("coo_to_csr_empty", "mx_coo_to_csr_begin", None, None, None, F64, 0, 4, 6, R, NFO)
case("coo_to_csr_logical", "mx_coo_to_csr_begin", CI, CJ, CL, LGL, 7, 4, 6, R, NFO)
case("coo_to_csr_none", "mx_coo_to_csr_begin", CI, CJ, None, NONE, 7, 4, 6, R, NFO)
case("coo_to_csr_none_empty", "mx_coo_to_csr_begin", None, None, None, NONE, 0, 4, 6, R, NFO)
# ---- mx_multiply_csr_by_coo_begin(logical, Xp, Xj, Xx, Yr, Yc, Yv, nnz_Y, max_row_X, max_col_X)
case("csr_by_coo", "mx_multiply_csr_by_coo_begin", 0, AP, AJ, AX, CI, CJ, CX, 7, 4, 6, R, NFO)
case("csr_by_coo_empty", "mx_multiply_csr_by_coo_begin", 0, AP, AJ, AX, I(1, 0, 3), I(0, 0, 5), D(1.0, 2.0, 3.0), 3, 4, 6, R,
     NFO)
case("csr_by_coo_no_entries", "mx_multiply_csr_by_coo_begin", 0, AP, AJ, AX, None, None, None, 0, 4, 6, R, NFO)
case("csr_by_coo_logical", "mx_multiply_csr_by_coo_begin", 1, AP, AJ, AL, CI, CJ, CL, 7, 4, 6, R, NFO)
# ---- mx_slice_coo_arbitrary_begin(ii, jj, xx, dtype, nnz, rows_base1, n_rows, cols_base1, n_cols, all_i, all_j,
#                                   i_is_seq, j_is_seq, i_is_rev_seq, j_is_rev_seq, nrows, ncols)
case("coo_slice_map", "mx_slice_coo_arbitrary_begin", CI, CJ, CX, F64, 7, I(3, 1, 3), 3, I(1), 1, 0, 1, 0, 0, 0, 0, 4, 6, R, NFO)
case("coo_slice_seq", "mx_slice_coo_arbitrary_begin", CI, CJ, CX, F64, 7, I(1, 2, 3), 3, I(6, 5, 4, 3), 4, 0, 0, 1, 0, 0, 1, 4,
     6, R, NFO)
case("coo_slice_empty", "mx_slice_coo_arbitrary_begin", CI, CJ, CX, F64, 7, I(2), 1, I(1, 6, 1), 3, 0, 0, 0, 0, 0, 0, 4, 6, R,
     NFO)
case("coo_slice_no_entries", "mx_slice_coo_arbitrary_begin", None, None, None, F64, 0, I(2), 1, I(1), 1, 0, 0, 0, 0, 0, 0, 4,
     6, R, NFO)
case("coo_slice_logical", "mx_slice_coo_arbitrary_begin", CI, CJ, CL, LGL, 7, I(3, 1, 3), 3, I(6, 1), 2, 0, 0, 0, 0, 0, 0, 4, 6,
     R, NFO)
case("coo_slice_none", "mx_slice_coo_arbitrary_begin", CI, CJ, None, NONE, 7, I(3, 1, 3), 3, I(1), 1, 0, 1, 0, 0, 0, 0, 4, 6, R,
     NFO)
case("coo_slice_none_empty", "mx_slice_coo_arbitrary_begin", CI, CJ, None, NONE, 7, I(2), 1, I(1), 1, 0, 1, 0, 0, 0, 0, 4, 6, R,
     NFO)
# ---- the compaction: mx_filter_sparse_begin(layout, p, nrows, idx0, idx1, x, dtype, nnz, mask) and the zero rules
ZV = D(1.5, 0.0, 3.0, NA_REAL, 0.0, 4.0)                          # A's values with zeros
M = I(1, 0, NA_INT, 1, 0, 1)
for lay, p, nr, i0, i1, tag in ((0, AP, 4, AJ, None, "csr"), (1, None, 0, AJ, I(5, 4, 3, 2, 1, 0), "coo"),
                                (2, None, 0, AJ, None, "svec")):
    case(f"filter_{tag}", "mx_filter_sparse_begin", lay, p, nr, i0, i1, AX, F64, 6, M, R, NFO)
    case(f"filter_{tag}_empty", "mx_filter_sparse_begin", lay, p, nr, i0, i1, AX, F64, 6, I(0, 0, 0, 0, 0, 0), R, NFO)
    case(f"filter_{tag}_all_kept", "mx_filter_sparse_begin", lay, p, nr, i0, i1, AL, LGL, 6, I(1, 1, 1, 1, 1, 1), R, NFO)
case("filter_svec_integer", "mx_filter_sparse_begin", 2, None, 0, AJ, None, I(3, 0, NA_INT, 1, 2, 0), I32, 6, M, R, NFO)
case("filter_csr_no_entries", "mx_filter_sparse_begin", 0, EP, 4, None, None, None, F64, 0, None, R, NFO)
for na_rm in (0, 1):
    case(f"zeros_csr_numeric_{na_rm}", "mx_remove_zero_valued_csr_numeric", AP, AJ, ZV, 4, na_rm, R, NFO)
    case(f"zeros_csr_logical_{na_rm}", "mx_remove_zero_valued_csr_logical", AP, AJ, AL, 4, na_rm, R, NFO)
    case(f"zeros_coo_numeric_{na_rm}", "mx_remove_zero_valued_coo_numeric", CI, CJ, D(0.5, 0.0, 4.0, 3.0, NA_REAL, 0.0, 1.0), 7,
         na_rm, R, NFO)
    case(f"zeros_coo_logical_{na_rm}", "mx_remove_zero_valued_coo_logical", CI, CJ, CL, 7, na_rm, R, NFO)
    case(f"zeros_svec_numeric_{na_rm}", "mx_remove_zero_valued_svec_numeric", AJ, ZV, 6, na_rm, R, NFO)
    case(f"zeros_svec_integer_{na_rm}", "mx_remove_zero_valued_svec_integer", AJ, I(3, 0, NA_INT, 1, 2, 0), 6, na_rm, R, NFO)
    case(f"zeros_svec_logical_{na_rm}", "mx_remove_zero_valued_svec_logical", AJ, AL, 6, na_rm, R, NFO)
case("zeros_csr_alias", "mx_remove_zero_valued_csr_numeric", AP, AJ, D(1.5, -2.0, 3.0, 1.0, 0.5, 4.0), 4, 0, R, NFO)
case("zeros_coo_alias", "mx_remove_zero_valued_coo_numeric", CI, CJ, D(1, 2, 3, 4, 5, 6, 7), 7, 1, R, NFO)
case("zeros_svec_alias", "mx_remove_zero_valued_svec_logical", AJ, I(1, 1, 1, NA_INT, 1, 1), 6, 0, R, NFO)
case("zeros_csr_all_removed", "mx_remove_zero_valued_csr_numeric", AP, AJ, D(0, 0, 0, 0, 0, 0), 4, 0, R, NFO)
case("zeros_coo_all_removed", "mx_remove_zero_valued_coo_logical", CI, CJ, I(0, 0, 0, 0, 0, 0, 0), 7, 0, R, NFO)
case("zeros_svec_all_removed", "mx_remove_zero_valued_svec_integer", AJ, I(0, 0, 0, 0, 0, 0), 6, 1, R, NFO)
case("zeros_csr_no_entries", "mx_remove_zero_valued_csr_numeric", EP, None, None, 4, 0, R, NFO)


def main(only):
    record = {}
    if only:
        with open(PATH) as f:
            record = json.load(f)
    for name, (fn, args) in CASES.items():
        if only and name not in only:
            continue
        got = run_call(fn, args)
        if got["status"] != 0 or got["finish"] != 0:
            print(f"{name}: the call failed and is not recorded: {got}")
            if "illegal" in got.get("error", "") or "fault" in got.get("error", ""):
                sys.exit("the device faulted: stopping, nothing written")
            continue
        record[name] = {"call": [fn, args], "result": got}
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}"
                                   for k, v in sorted(record.items())) + "\n}\n")
    print(f"{PATH}: {len(record)} calls, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
