"""CPU model of the one-triangle sparse x sparse product of include/mxgpu_gram.h, exact in pattern
and bits, on top of tests/spgemm_model.py.

The products are those of SM.expand; the keep rule drops the ones outside the triangle; SM.fold folds what is left.
Every cell is folded on its own, in the same order as in the full product, so the result is the triangle of
SM.spgemm bit for bit (tests/test_gram_model.py checks that).  Beside it: the two product counts the count pass can
report, the masked row bounds ub_i = min(f_i, w_i) from which the bins are chosen, the mean step length that chooses a
lane width, and a stable CSR transpose."""
import numpy as np

import spgemm_model as SM

UPPER, LOWER = 0, 1                     # mx_uplo (include/mxgpu_sym.h)


def keep(uplo, rows, cols):
    """the keep rule: upper keeps a product for cell (i, j) when j >= i, lower when j <= i"""
    return cols >= rows if uplo == UPPER else cols <= rows


def window(uplo, m, n):
    """w_i, the number of columns the mask leaves row i of an m x n result"""
    i = np.arange(m, dtype=np.int64)
    return np.maximum(0, n - i) if uplo == UPPER else np.minimum(i + 1, n)


def spgemm_tri(Ap, Aj, Ax, Bp, Bj, Bx, K, n, uplo):
    """(indptr, indices, values) of the triangle `uplo` of A B"""
    rows, cols, t = SM.expand(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    k = keep(uplo, rows, cols)
    return SM.fold(rows[k], cols[k], t[k], np.asarray(Ap).size - 1)


def triangle_of(p, j, x, uplo):
    """the entries of a CSR that lie in the triangle, as a CSR"""
    m = p.size - 1
    rows = np.repeat(np.arange(m), np.diff(p))
    k = keep(uplo, rows, j)
    out = np.zeros(m + 1, dtype=np.int32)
    out[1:] = np.cumsum(np.bincount(rows[k], minlength=m))
    return out, j[k], x[k]


def _step_lengths(Ap, Aj, Bp, Bj, K, uplo, b_sorted):
    """per entry of A: its row, and how many entries of its row of B a step reads: all of them, or with b_sorted the
    ones the trim leaves (upper: columns >= i, lower: columns <= i; B's rows ascending)"""
    Ap, Aj, Bp, Bj = (np.asarray(a, dtype=np.int64) for a in (Ap, Aj, Bp, Bj))
    m = Ap.size - 1
    rows_a = np.repeat(np.arange(m), np.diff(Ap))
    ok = (Aj >= 0) & (Aj < K)
    k = np.where(ok, Aj, 0)
    lens = np.where(ok, Bp[k + 1] - Bp[k], 0) if Bp.size > 1 else np.zeros(Aj.size, np.int64)
    if b_sorted:
        q = np.flatnonzero(lens > 0)
        src = np.repeat(q, lens[q])
        first = np.cumsum(lens[q]) - lens[q]
        pos = np.repeat(Bp[k[q]], lens[q]) + np.arange(int(lens[q].sum())) - np.repeat(first, lens[q])
        inside = keep(uplo, rows_a[src], Bj[pos])
        lens = np.bincount(src[inside], minlength=Aj.size).astype(np.int64)
    return rows_a, ok, lens


def products(Ap, Aj, Bp, Bj, K, uplo, b_sorted):
    """what the count pass reports in *products_host: every product of the rows, or with b_sorted the ones inside the
    window (columns outside [0, n) that the trim leaves are counted: the bounds pass does not look at them)"""
    return int(_step_lengths(Ap, Aj, Bp, Bj, K, uplo, b_sorted)[2].sum())


def row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, b_sorted):
    """ub_i = min(f_i, w_i) per row"""
    m = np.asarray(Ap).size - 1
    rows_a, _, lens = _step_lengths(Ap, Aj, Bp, Bj, K, uplo, b_sorted)
    f = np.bincount(rows_a, weights=lens, minlength=m).astype(np.int64)
    return np.minimum(f, window(uplo, m, n))


def mean_step(Ap, Aj, Bp, Bj, K, uplo, b_sorted):
    """ceil(f_i / the row's entries with a column inside [0, K)): what chooses the lane width of a lane-group row
    (<= 8, <= 16, else 32); 0 where the row has no such entry"""
    m = np.asarray(Ap).size - 1
    rows_a, ok, lens = _step_lengths(Ap, Aj, Bp, Bj, K, uplo, b_sorted)
    f = np.bincount(rows_a, weights=lens, minlength=m).astype(np.int64)
    used = np.bincount(rows_a[ok], minlength=m).astype(np.int64)
    return np.where(used > 0, -(-f // np.maximum(used, 1)), 0)


def transpose(p, j, x, ncol):
    """(indptr, indices, values) of the CSR of X^T, stable: the rows ascending inside every row of the result, as
    mxd_csr_column_order + mxd_csr_transpose_by_order give it"""
    p, j = np.asarray(p, dtype=np.int64), np.asarray(j, dtype=np.int64)
    rows = np.repeat(np.arange(p.size - 1), np.diff(p))
    order = np.argsort(j, kind="stable")
    tp = np.zeros(ncol + 1, dtype=np.int32)
    tp[1:] = np.cumsum(np.bincount(j, minlength=ncol))
    return tp, rows[order].astype(np.int32), None if x is None else np.asarray(x)[order]


def sort_rows(p, j, x):
    """the CSR with every row ascending (stable)"""
    rows = np.repeat(np.arange(np.asarray(p).size - 1), np.diff(p))
    order = np.lexsort((np.asarray(j), rows))
    return p, np.asarray(j)[order], None if x is None else np.asarray(x)[order]


def gram(p, j, x, dims, trans, uplo):
    """the triangle `uplo` of X X^T (trans false) or X^T X for the CSR arrays of X: what mx_csr_gram_begin returns"""
    nrow, ncol = dims
    tp, tj, tx = transpose(p, j, x, ncol)
    if trans:
        return spgemm_tri(tp, tj, tx, p, j, x, nrow, ncol, uplo)
    return spgemm_tri(p, j, x, tp, tj, tx, ncol, nrow, uplo)
