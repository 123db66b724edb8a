#!/usr/bin/env python3
"""Generates tests/golden/reference_golden.npz: seeded inputs and what the REFERENCE's own compiled C++ returns for
them (oracle/ref.py over oracle/_ref/libmxref.so, built by `make -C oracle ref`).  The file holds data only: inputs,
outputs, alias flags, messages, the seeds and the compile flags.  Shapes are the smallest that reach every branch.
Run from the repo root:  python tests/golden/make_reference_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dvec_na_model as DM  # noqa: E402
import refpin  # noqa: E402
from conftest import rand_csr  # noqa: E402
from oracle import ref as Ref  # noqa: E402

NA = np.int32(-2147483648)
NA_REAL, NAN2 = DM.NA_REAL, DM.OTHER_NAN
SEED = 20240
records = []


def rec(fn, *args, label=""):
    records.append(refpin.capture(Ref, fn, args, label))
    return records[-1]


def i32(a):
    return np.asarray(a, dtype=np.int32)


def rng(k):
    return np.random.default_rng(SEED + k)


def lgl(n, k, na=0.2):
    return rng(k).choice(i32([0, 1, NA]), size=n, p=[(1 - na) / 2, (1 - na) / 2, na])


# ---- SpMM (n <= m for the column-major CSR x dense exports: scratch overflow in the reference, matmul.cpp:176)
for name, (m, K, n, dens) in {"a": (40, 30, 20, 0.3), "row1": (1, 12, 1, 0.6), "col1": (9, 1, 3, 1.0)}.items():
    p, j, x = rand_csr(m, K, dens, seed=SEED + m, sorted_cols=False, empty_rows=(0,) if m > 3 else ())
    Y = np.asfortranarray(rng(n).normal(size=(n, K)).round(3))
    rec("tcrossprod_csr_dense_numeric", p, j, x, Y, 1, label=name)
    rec("tcrossprod_csr_dense_float32", p, j, x, Y.astype(np.float32), 1, label=name)
    for nn in (n, m + 3):                                   # dense * sparse has no such limit: also n > m
        X = np.asfortranarray(rng(nn + 1).normal(size=(nn, K)).round(3))
        rec("matmul_dense_csc_numeric", X, p, j, x, 1, label=f"{name}_{nn}")
        rec("matmul_dense_csc_float32", X.astype(np.float32), p, j, x, 1, label=f"{name}_{nn}")
        rec("tcrossprod_dense_csr_numeric", X, p, j, x, 1, K, label=f"{name}_{nn}")
        rec("tcrossprod_dense_csr_float32", X.astype(np.float32), p, j, x, 1, K, label=f"{name}_{nn}")

# ---- SpMV and CSR %*% sparse vector, every kind, NA entries
p, j, x = rand_csr(30, 12, 0.4, seed=SEED + 77, sorted_cols=False, empty_rows=(4,))
yd = rng(78).normal(size=12).round(3)
yi = rng(79).integers(-9, 9, size=12).astype(np.int32); yi[[2, 7]] = NA
yl = lgl(12, 80)
rec("matmul_csr_dvec_numeric", p, j, x, yd, 1)
rec("matmul_csr_dvec_integer", p, j, x, yi, 1)
rec("matmul_csr_dvec_logical", p, j, x, yl, 1)
rec("matmul_csr_dvec_float32", p, j, x, yd.astype(np.float32), 1)
ps, js, xs = rand_csr(30, 12, 0.4, seed=SEED + 81, empty_rows=(4,))
si = i32([2, 3, 7, 8, 12])
rec("matmul_csr_svec_numeric", ps, js, xs, si, np.array([1.5, -2.0, NA_REAL, 0.25, 3.0]), 1)
rec("matmul_csr_svec_integer", ps, js, xs, si, i32([3, NA, -1, 0, 7]), 1)
rec("matmul_csr_svec_logical", ps, js, xs, si, i32([1, NA, 0, 1, 1]), 1)
rec("matmul_csr_svec_binary", ps, js, xs, si, 1)
rec("matmul_csr_svec_float32", ps, js, xs, si, np.array([1.5, -2.0, np.nan, 0.25, 3.0], dtype=np.float32), 1)

# ---- CSR (+ - * | xor &) CSR: general, disjoint, one empty, cancelling, special values, shared objects
a = rand_csr(25, 14, 0.4, seed=SEED + 5, empty_rows=(3,)); b = rand_csr(25, 14, 0.5, seed=SEED + 6, empty_rows=(3, 9))
xa = a[2].copy(); xa[:5] = [np.inf, -np.inf, NA_REAL, 0.0, -0.0]
xb = b[2].copy(); xb[:4] = [-np.inf, 0.0, NAN2, -0.0]
for label, (A, B) in {"general": ((a[0], a[1], xa), (b[0], b[1], xb)),
                      "one_empty": (rand_csr(10, 8, 0.0, seed=1), rand_csr(10, 8, 0.5, seed=SEED + 2)),
                      "cancel": ((a[0], a[1], xa), (a[0].copy(), a[1].copy(), -xa))}.items():
    rec("add_csr_elemwise", A[0], B[0], A[1], B[1], A[2], B[2], False, label=label)
    rec("add_csr_elemwise", A[0], B[0], A[1], B[1], A[2], B[2], True, label=label)
    rec("multiply_csr_elemwise", A[0], B[0], A[1], B[1], A[2], B[2], label=label)
rec("add_csr_elemwise", a[0], a[0], a[1], a[1], xa, xb[:xa.size] if xb.size >= xa.size else xa * 2, False, label="same_structure")
rec("add_csr_elemwise", a[0], a[0], a[1], a[1], xa, xa, True, label="same_everything")
rec("multiply_csr_elemwise", a[0], a[0], a[1], a[1], xa, xa, label="same_structure")
l1 = rand_csr(20, 9, 0.5, seed=SEED + 31, dtype="l"); l2 = rand_csr(20, 9, 0.5, seed=SEED + 32, dtype="l")
rec("logicalor_csr_elemwise", l1[0], l2[0], l1[1], l2[1], l1[2], l2[2], False)
rec("logicalor_csr_elemwise", l1[0], l2[0], l1[1], l2[1], l1[2], l2[2], True)
rec("logicaland_csr_elemwise", l1[0], l2[0], l1[1], l2[1], l1[2], l2[2])
rec("logicalor_csr_elemwise", l1[0], l1[0], l1[1], l1[1], l1[2], l1[2][::-1].copy(), True, label="same_structure")
rec("logicaland_csr_elemwise", l1[0], l1[0], l1[1], l1[1], l1[2], l1[2][::-1].copy(), label="same_structure")

# ---- row gather, column slices, reversals
p, j, x = rand_csr(50, 20, 0.2, seed=SEED + 41, empty_rows=(10, 11))
xl = lgl(j.size, 42)
rows = i32([49, 49, 10, 0, 7, 7, 3, 11, 48])
for rr, label in ((rows, "repeats"), (i32([10, 11, 10]), "nothing")):
    rec("copy_csr_rows_numeric", p, j, x, rr, label=label)
    rec("copy_csr_rows_logical", p, j, xl, rr, label=label)
    rec("copy_csr_rows_binary", p, j, rr, label=label)
for index1 in (False, True):
    cols = np.arange(5, 14, dtype=np.int32) + int(index1)
    rec("copy_csr_rows_col_seq_numeric", p, j, x, rows, cols, index1)
    rec("copy_csr_rows_col_seq_logical", p, j, xl, rows, cols, index1)
    rec("copy_csr_rows_col_seq_binary", p, j, rows, cols, index1)
cols = i32([19, 0, 7, 7, 3, 12, 7])
rec("copy_csr_arbitrary_numeric", p, j, x, rows, cols)
rec("copy_csr_arbitrary_logical", p, j, xl, rows, cols)
rec("copy_csr_arbitrary_binary", p, j, rows, cols)
rec("reverse_rows_numeric", p, j, x)
rec("reverse_rows_logical", p, j, xl)
rec("reverse_rows_binary", p, j)
rec("reverse_columns_inplace_numeric", p, j, x, 20)
rec("reverse_columns_inplace_logical", p, j, xl, 20)
rec("reverse_columns_inplace_binary", p, j, 20)
for v in ([3, 4, 5], [5, 4, 3], [3, 5, 6], [7], [2, 2]):
    rec("check_is_seq", i32(v))
    rec("check_is_rev_seq", i32(v))

# ---- cbind / rbind
A = rand_csr(12, 6, 0.4, seed=SEED + 51, empty_rows=(2,)); B = rand_csr(9, 5, 0.5, seed=SEED + 52)
rec("cbind_csr_numeric", A[0], A[1], A[2], B[0], B[1] + 6, B[2])
rec("cbind_csr_numeric", B[0], B[1], B[2], A[0], A[1] + 5, A[2], label="shorter_first")
rec("cbind_csr_logical", A[0], A[1], lgl(A[1].size, 53), B[0], B[1] + 6, lgl(B[1].size, 54))
rec("cbind_csr_binary", A[0], A[1], B[0], B[1] + 6)
rec("concat_indptr2", A[0], B[0])
objs = [(0, A[0], A[1], A[2]), (1, B[0], B[1], lgl(B[1].size, 55)), (2, B[0], B[1], None),
        (3, None, i32([1, 4]), np.array([1.5, NA_REAL])), (4, None, i32([2, 3, 6]), i32([5, NA, 0])),
        (5, None, i32([1, 2, 5]), i32([1, NA, 0])), (6, None, i32([3]), None)]
nr = i32([12, 9, 9, 1, 1, 1, 1])
for out_kind in (0, 1, 2):
    flat = [o[k] for o in objs for k in (1, 2, 3)]
    rec("concat_csr_batch", i32([o[0] for o in objs]), nr, out_kind, *flat, label=f"out{out_kind}")

# ---- CSR (.) dense matrix
p, j, x = rand_csr(11, 7, 0.45, seed=SEED + 61, empty_rows=(5,))
x = x.copy(); x[:4] = [np.inf, NA_REAL, -0.0, 0.0]
D = rng(62).normal(size=(11, 7)).round(2); D[0, :] = [np.nan, np.inf, 0.0, -0.0, 1.0, -1.0, NA_REAL]
Di = rng(63).integers(-4, 5, size=(11, 7)).astype(np.int32); Di[rng(64).random((11, 7)) < 0.15] = NA
rec("multiply_csr_by_dense_elemwise_double", p, j, x, np.asfortranarray(D))
rec("multiply_csr_by_dense_elemwise_float32", p, j, x, np.asfortranarray(D.astype(np.float32)))
rec("multiply_csr_by_dense_elemwise_int", p, j, x, np.asfortranarray(Di))
rec("multiply_csr_by_dense_elemwise_bool", p, j, x, np.asfortranarray(lgl(77, 65).reshape(11, 7)))
rec("logicaland_csr_by_dense_cpp", p, j, lgl(j.size, 66), np.asfortranarray(lgl(77, 67).reshape(11, 7)))

# ---- CSR (op) dense vector, values only: 5 ops x both orders x the length branches, special values
p, j, x = rand_csr(12, 7, 0.45, seed=SEED + 71, empty_rows=(5,))
x = x.copy(); x[:4] = [np.inf, -np.inf, np.nan, -0.0]
xl = lgl(j.size, 72)
for vname, ln in {"nrows": 12, "full": 84, "divides": 4, "general": 5, "one": 1, "between": 30}.items():
    v = (rng(73 + ln).uniform(0.5, 3.0, size=ln) * rng(74 + ln).choice([-1.0, 1.0], size=ln)).round(3)
    for o, opname in enumerate(refpin.OPS):
        for lhs in (True, False):
            rec("multiply_csr_by_dvec_no_NAs_numeric", p, j, x, v, 7, *[k == o for k in range(5)], lhs, label=f"{opname}_{vname}")
    vl = lgl(ln, 75 + ln)
    rec("logicaland_csr_by_dvec_internal", p, j, xl, vl, 7, label=vname)
rec("multiply_csr_by_dvec_no_NAs_numeric", p, j, x, np.ones(12), 7, False, False, False, False, False, True, label="no_flag")

# ---- %% %/% ^ where the reference's long double step is not exact: quotients spread over 1 .. 2^52, quotients
#      one ulp from an integer, the fabs(x2) * LDBL_EPSILON > 1 branch, and ^'s table of special values
m = 400
pa = np.arange(m + 1, dtype=np.int32); ja = np.zeros(m, dtype=np.int32)
r = rng(90)
x2 = (r.uniform(0.05, 9.0, size=m) * r.choice([-1.0, 1.0], size=m))
x1 = x2 * np.exp2(r.uniform(0, 52, size=m)) * r.uniform(1.0, 2.0, size=m) * r.choice([-1.0, 1.0], size=m)
edge = [(0.3, 0.1), (0.9, 0.3), (1.0, 0.1), (-0.3, 0.1), (0.3, -0.1), (-0.9, 0.3), (0.9, -0.3), (-1.0, 0.1), (1.0, -0.1),
        (-0.3, -0.1), (-0.9, -0.3), (-1.0, -0.1), (5.0, 2.0 ** 70), (-5.0, 2.0 ** 70), (5.0, -2.0 ** 70), (2.0 ** 70, 2.0 ** 70),
        (2.0 ** 69, -2.0 ** 70), (np.inf, 2.0 ** 70), (0.0, 2.0 ** 70), (1e300, 3.0), (7.0, 0.0), (-7.0, 0.0), (0.0, 0.0),
        (np.inf, 2.0), (2.0, np.inf), (-2.0, np.inf), (2.0, -np.inf), (np.nan, 2.0), (2.0, NA_REAL), (1e-300, 7.0),
        (6.0, 3.0), (-6.0, 3.0), (5.5, -2.0), (2.0 ** 53 + 2, 3.0), (2.0 ** 60, 7.0)]
for k, (u, w) in enumerate(edge):
    x1[k], x2[k] = u, w
for o, opname in ((3, "mod"), (4, "idiv")):
    for lhs in (True, False):
        rec("multiply_csr_by_dvec_no_NAs_numeric", pa, ja, x1 if lhs else x2, x2 if lhs else x1, 1,
            *[k == o for k in range(5)], lhs, label=f"{opname}_quotients")
pw = [(1.0, np.nan), (np.nan, 0.0), (0.0, 2.5), (0.0, -2.5), (0.0, np.nan), (-0.0, -3.0), (np.inf, -1.0), (np.inf, 2.0), (-np.inf, 3.0),
      (-np.inf, 4.0), (-np.inf, -3.0), (-np.inf, 0.5), (-np.inf, np.inf), (0.5, np.inf), (2.0, np.inf), (0.5, -np.inf), (2.0, -np.inf),
      (-2.0, np.inf), (-2.0, 0.5), (-2.0, 3.0), (-1.5, 2.0), (NA_REAL, 2.0), (2.0, NA_REAL), (1.0, np.inf), (-1.0, np.inf),
      (3.0, 2.0), (2.5, 10.5), (10.0, -3.0), (1e200, 2.0), (1.0000001, 1e9)]
b1 = np.concatenate([[u for u, _ in pw], r.uniform(0.1, 30.0, size=m - len(pw))])
b2 = np.concatenate([[w for _, w in pw], r.uniform(-20.0, 20.0, size=m - len(pw)).round(1)])
for lhs in (True, False):
    rec("multiply_csr_by_dvec_no_NAs_numeric", pa, ja, b1 if lhs else b2, b2 if lhs else b1, 1, False, True, False, False, False,
        lhs, label="pow_table")

# ---- CSR (op) dense vector keeping NA cells: row-ruled and flat regimes, clean and dirty X, every special of the pools
for o, op in enumerate(DM.OPS):
    fl = [k == o for k in range(5)]
    p, j, x = DM.make_csr(24, 9, 0.35, SEED + 100 + o, empty_rows=(3,), full_rows=(5,), positive=(op == "^"))
    for L, label in ((24, "rows"), (8, "divides"), (1, "one"), (7, "flat"), (216, "full"), (50, "flat_between")):
        v = DM.make_vector(L, op, SEED + 110 + o + L, at=(0, L - 1), share=0.25 if L > 1 else 0.0)
        rec("multiply_csr_by_dvec_with_NAs", p, j, x, v, 9, *fl, True, label=f"{op}_{label}")
    v = DM.make_vector(7, op, SEED + 120, share=0.0); v[:] = np.abs(v) + 1.0
    rec("multiply_csr_by_dvec_with_NAs", p, j, x, v, 9, *fl, True, label=f"{op}_flat_nothing_added")
    for flat in (False, True):
        dp, dj, dx, dv, dn = DM.dirty_case(op, flat)
        rec("multiply_csr_by_dvec_with_NAs", dp[:16], dj[:dp[15]], dx[:dp[15]], dv[:15] if not flat else dv[:11], dn, *fl, True,
            label=f"{op}_dirty_{'flat' if flat else 'rows'}")
p, j, x = DM.make_csr(24, 9, 0.35, SEED + 130, empty_rows=(3,))
for o in (0, 4):
    v = DM.make_vector(8, DM.OPS[o], SEED + 131 + o, at=(0, 7), share=0.25)
    rec("multiply_csr_by_dvec_with_NAs", p, j, x, v, 9, *[k == o for k in range(5)], False, label=f"{DM.OPS[o]}_rhs")

# ---- CSR * sparse vector (sorted 1-based ii, recycled every `length` rows)
p, j, x = rand_csr(18, 8, 0.4, seed=SEED + 140, empty_rows=(6,))
x = x.copy(); x[::7] = np.nan; x[3::11] = np.inf; x[5::13] = 0.0; x[1::17] = NA_REAL
ii = i32([1, 2, 4, 5, 7, 8, 9])
xv = np.array([2.0, NA_REAL, np.inf, 0.0, -1.5, NAN2, -np.inf])
for length, label in ((18, "whole"), (9, "recycled"), (6, "recycled6")):
    k = int(np.searchsorted(ii, length, side="right"))
    rec("multiply_csr_by_svec_no_NAs", p, j, x, ii[:k], xv[:k], length, label=label)
    rec("multiply_csr_by_svec_keep_NAs", p, j, x, ii[:k], xv[:k], 8, length, label=label)
    rec("multiply_csr_by_svec_no_NAs", p, j, x, ii[:k], np.zeros(0), length, label=label + "_pattern")
    rec("multiply_csr_by_svec_keep_NAs", p, j, x, ii[:k], np.zeros(0), 8, length, label=label + "_pattern")
rec("multiply_csr_by_svec_no_NAs", p, j, x, i32([]), np.zeros(0), 18, label="empty_vector")
rec("multiply_csr_by_svec_keep_NAs", p, j, x, i32([]), np.zeros(0), 8, 18, label="empty_vector")

# ---- CSC (.) dense matrix, ignoring and keeping the dense NA cells (rows sorted inside each column)
p, i, x = rand_csr(9, 13, 0.35, seed=SEED + 150, empty_rows=(2,))           # 9 columns of 13 rows
x = x.copy(); x[::6] = np.nan; x[2::9] = np.inf; x[4::10] = 0.0
D = rng(151).normal(size=(13, 9)).round(2)
D[rng(152).random((13, 9)) < 0.12] = NA_REAL; D[rng(153).random((13, 9)) < 0.06] = NAN2; D[1, 1] = np.inf; D[2, 3] = 0.0
Di = rng(154).integers(-4, 5, size=(13, 9)).astype(np.int32); Di[rng(155).random((13, 9)) < 0.15] = NA
Dl = lgl(117, 156).reshape(13, 9)
Df = D.astype(np.float32)
xl = lgl(i.size, 157)
for kind, dense in (("numeric", D), ("float32", Df), ("integer", Di), ("logical", Dl)):
    rec(f"multiply_csc_by_dense_ignore_NAs_{kind}", p, i, x, np.asfortranarray(dense))
    rec(f"multiply_csc_by_dense_keep_NAs_{kind}", p, i, x, np.asfortranarray(dense))
rec("logicaland_csc_by_dense_ignore_NAs", p, i, xl, np.asfortranarray(Dl))
rec("multiply_csc_by_dense_keep_NAs_numeric", p, i, x, np.asfortranarray(np.abs(np.nan_to_num(D)) + 1.0), label="nothing_added")

# ---- CSR (.) COO
p, j, x = rand_csr(15, 10, 0.4, seed=SEED + 160, empty_rows=(7,))
r = rng(161)
ci, cj = r.integers(0, 17, size=60).astype(np.int32), r.integers(0, 12, size=60).astype(np.int32)
cv = r.normal(size=60).round(2); cv[::9] = np.nan; cv[1::13] = 0.0
rec("multiply_csr_by_coo_elemwise", p, j, x, ci, cj, cv, 15, 10)
rec("logicaland_csr_by_coo_elemwise", p, j, lgl(j.size, 162), ci, cj, lgl(60, 163), 15, 10)
for o, opname in enumerate(refpin.OPS):
    vv = (r.uniform(0.5, 3.0, size=7) * r.choice([-1.0, 1.0], size=7)).round(3)
    rec("multiply_coo_by_dense_ignore_NAs_numeric", ci, cj, np.abs(cv) + 0.5 if opname == "pow" else cv, vv, 17, 12,
        *[k == o for k in range(5)], True, label=opname)
rec("multiply_coo_by_dense_ignore_NAs_logical", ci, cj, lgl(60, 164), lgl(17, 165), 17, 12)

# ---- remove_zero_valued_*: with and without na.rm; nothing to remove returns the inputs themselves
p, j, _ = rand_csr(14, 9, 0.45, seed=SEED + 170, empty_rows=(4,))
xd = rng(171).choice(np.array([0.0, -0.0, 1.5, -2.0, NA_REAL, NAN2, np.inf]), size=j.size)
xl = lgl(j.size, 172, na=0.3)
xi = rng(173).choice(i32([0, 3, -4, NA]), size=j.size)
rr = np.repeat(np.arange(14, dtype=np.int32), np.diff(p))
for na_rm in (False, True):
    rec("remove_zero_valued_csr_numeric", p, j, xd, na_rm)
    rec("remove_zero_valued_csr_logical", p, j, xl, na_rm)
    rec("remove_zero_valued_coo_numeric", rr, j, xd, na_rm)
    rec("remove_zero_valued_coo_logical", rr, j, xl, na_rm)
    rec("remove_zero_valued_svec_numeric", j + 1, xd, na_rm)
    rec("remove_zero_valued_svec_integer", j + 1, xi, na_rm)
    rec("remove_zero_valued_svec_logical", j + 1, xl, na_rm)
    rec("remove_zero_valued_csr_numeric", p, j, np.abs(np.nan_to_num(xd, posinf=3.0)) + 1.0, na_rm, label="nothing_removed")
    rec("remove_zero_valued_csr_logical", p, j, np.ones(j.size, dtype=np.int32), na_rm, label="nothing_removed")
    rec("remove_zero_valued_coo_numeric", rr, j, np.abs(np.nan_to_num(xd, posinf=3.0)) + 1.0, na_rm, label="nothing_removed")
    rec("remove_zero_valued_svec_numeric", j + 1, np.abs(np.nan_to_num(xd, posinf=3.0)) + 1.0, na_rm, label="nothing_removed")

# ---- validity checks: every message, in the order the reference tests them
good_p, good_j = i32([0, 2, 2, 5]), i32([0, 3, 1, 2, 3])
for label, (pp, jj) in {"valid": (good_p, good_j), "negative": (good_p, i32([0, 3, -1, 2, 3])), "too_large": (good_p, i32([0, 4, 1, 2, 3])),
                        "na_index": (good_p, i32([0, 3, NA, 2, 3])), "na_pointer": (i32([0, NA, 2, 5]), good_j),
                        "decreasing": (i32([0, 3, 2, 5]), good_j), "negative_and_large": (good_p, i32([9, 3, -1, 2, 3]))}.items():
    rec("check_valid_csr_matrix", pp, jj, 3, 4, label=label)
for label, (a_, b_) in {"valid": ([0, 2, 1], [3, 0, 1]), "neg_i": ([0, -2, 1], [3, 0, 1]), "big_i": ([0, 3, 1], [3, 0, 1]),
                        "na_i": ([0, NA, 1], [3, 0, 1]), "neg_j": ([0, 2, 1], [3, -1, 1]), "big_j": ([0, 2, 1], [4, 0, 1]),
                        "na_j": ([0, 2, 1], [3, NA, 1])}.items():
    rec("check_valid_coo_matrix", i32(a_), i32(b_), 3, 4, label=label)
for label, a_ in {"valid": [1, 3, 5], "negative": [1, -3, 5], "last_position": [1, 3, 6], "too_large": [1, 3, 7], "na": [1, NA, 5],
                  "zero": [0, 3, 5]}.items():       # the 1-based @i against the length: the last position fails in the reference
    rec("check_valid_svec", i32(a_), 6, label=label)
p, j, _ = rand_csr(14, 9, 0.45, seed=SEED + 180, empty_rows=(4, 13))
rec("rebuild_indptr_after_filter", p, lgl(j.size, 181))

# ---- index sorts (in place)
p, j, x = rand_csr(16, 12, 0.4, seed=SEED + 190, sorted_cols=False, empty_rows=(2,))
rec("sort_sparse_indices_numeric", p, j, x)
rec("check_indices_are_sorted", p, j, label="unsorted")                # the per-row check_is_sorted that gates the sort
rec("check_indices_are_sorted", p, np.concatenate([np.sort(j[p[r]:p[r + 1]]) for r in range(16)]).astype(np.int32), label="sorted")
rec("check_indices_are_sorted", i32([0, 0, 1, 3]), i32([5, 2, 2]), label="repeat_counts_as_sorted")
rec("sort_sparse_indices_logical", p, j, lgl(j.size, 191))
rec("sort_sparse_indices_binary", p, j)
perm = rng(192).permutation(40).astype(np.int32)[:25] + 1
rec("sort_vector_indices_numeric", perm, rng(193).normal(size=25).round(2))
rec("sort_vector_indices_integer", perm, rng(194).integers(-5, 5, size=25).astype(np.int32))
rec("sort_vector_indices_logical", perm, lgl(25, 195))
rec("sort_vector_indices_binary", perm)
rec("sort_vector_indices_numeric", np.sort(perm), rng(196).normal(size=25).round(2), label="sorted_already")

# ---- COO slicing: sequence, reversed sequence, no repeats, repeats; one side whole; single cells
r = rng(200)
ti, tj = r.integers(0, 20, size=90).astype(np.int32), r.integers(0, 15, size=90).astype(np.int32)
tx = r.normal(size=90).round(2); tl = lgl(90, 201)
sel = {"seq": (np.arange(4, 12), np.arange(2, 9)), "rev": (np.arange(12, 4, -1), np.arange(9, 2, -1)),
       "norepeat": (i32([9, 2, 17, 5, 20]), i32([15, 1, 7, 3])), "repeat": (i32([9, 2, 9, 5, 2, 20]), i32([7, 1, 7, 7, 3]))}
for label, (ri, cj_) in sel.items():
    ri, cj_ = i32(ri), i32(cj_)
    fl = (label == "seq", label == "seq", label == "rev", label == "rev")
    rec("slice_coo_arbitrary_numeric", ti, tj, tx, ri, cj_, False, False, *fl, 20, 15, label=label)
    rec("slice_coo_arbitrary_logical", ti, tj, tl, ri, cj_, False, False, *fl, 20, 15, label=label)
    rec("slice_coo_arbitrary_binary", ti, tj, ri, cj_, False, False, *fl, 20, 15, label=label)
    rec("slice_coo_arbitrary_numeric", ti, tj, tx, ri, np.arange(1, 16, dtype=np.int32), False, True, fl[0], False, fl[2], False, 20, 15,
        label=label + "_all_j")     # a whole side is the full 1..n sequence; all_i also sets i_is_seq, all_j leaves j_is_seq unset
    rec("slice_coo_arbitrary_numeric", ti, tj, tx, np.arange(1, 21, dtype=np.int32), cj_, True, False, True, fl[1], False, fl[3], 20, 15,
        label=label + "_all_i")
for (a_, b_) in ((int(ti[5]), int(tj[5])), (int(ti[40]), int(tj[40])), (19, 14), (0, 0)):
    rec("slice_coo_single_numeric", ti, tj, tx, a_, b_)
    rec("slice_coo_single_logical", ti, tj, tl, a_, b_)
    rec("slice_coo_single_binary", ti, tj, a_, b_)

for r_ in records:      # the undefined half of this routine's doubles is dropped: see refpin.CSR_LOGICAL_VALUES_ARE_LOGICALS
    if r_.fn == refpin.CSR_LOGICAL_VALUES_ARE_LOGICALS and "values" not in r_.alias:
        r_.out["values"] = refpin.defined_values(r_.out["values"])
        r_.label += "defined_half_of_values"

refpin.save(records, dict(seed=SEED, compile_flags=Ref.compile_flags(),
                          source="outputs of the reference's own translation units behind oracle/refshim",
                          not_reference_run="R_pow belongs to R, not to the reference (its copy is commented out, "
                                            "operators.cpp:1555-1598); every ^ value here comes from the stand-in's "
                                            "R_pow (oracle/refshim/refshim.cpp). For ^ the records pin operand order, "
                                            "recycling and the fill cells only."))
errs = [r for r in records if r.err is not None]
print(f"wrote {refpin.PATH}: {len(records)} records ({len(errs)} stops), {os.path.getsize(refpin.PATH)} bytes")
for r in errs:
    print("  stop:", r, "->", r.err)
