"""CPU model of the sparse x sparse product of include/mxgpu_spgemm.h, exact in pattern and bits.

The products are expanded in (A storage order, B storage order), sorted stably by (row, column), and every run is
folded left to right: the first product as it is, then fl(sum + product).  That is the order the header defines, so the
device result must equal this one bit for bit.  The fold is vectorised by the rank of a product within its run."""
import numpy as np

NA_INT = np.int32(-2**31)
NA_REAL = np.frombuffer(np.uint64(0x7FF00000000007A2).tobytes(), dtype=np.float64)[0]


def as_double(x, nnz):
    """the values of an operand as the product reads them: f64 as is, int32 R logicals as 0 / 1 with NA -> NA_real_,
    None (a pattern) as ones"""
    if x is None:
        return np.ones(nnz)
    x = np.asarray(x)
    if x.dtype == np.float64:
        return x
    assert x.dtype == np.int32
    return np.where(x == NA_INT, NA_REAL, (x != 0).astype(np.float64))


def expand(Ap, Aj, Ax, Bp, Bj, Bx, K, n):
    """(row, column, product) of every product, in (A storage order, B storage order); an A column outside [0, K) gives
    none, a B column outside [0, n) is skipped"""
    Ap, Aj, Bp, Bj = (np.asarray(a, dtype=np.int64) for a in (Ap, Aj, Bp, Bj))
    m = Ap.size - 1
    a, b = as_double(Ax, Aj.size), as_double(Bx, Bj.size)
    rows_a = np.repeat(np.arange(m), np.diff(Ap))
    q = np.flatnonzero((Aj >= 0) & (Aj < K))
    k = Aj[q]
    lens = Bp[k + 1] - Bp[k]
    src = np.repeat(q, lens)
    first = np.cumsum(lens) - lens
    pos = np.repeat(Bp[k], lens) + np.arange(int(lens.sum())) - np.repeat(first, lens)
    cols = Bj[pos]
    ok = (cols >= 0) & (cols < n)
    src, pos, cols = src[ok], pos[ok], cols[ok]
    with np.errstate(all="ignore"):
        t = a[src] * b[pos]                         # one rounding per product
    return rows_a[src], cols, t


def by_cell(rows, cols):
    """the stable order by (row, column): one sort of a combined key, which a lexsort takes three times as long for"""
    width = int(cols.max()) + 1 if cols.size else 1
    return np.argsort(rows * width + cols, kind="stable")


def fold(rows, cols, t, m):
    """(indptr, indices, values) of the runs of equal (row, column), each folded left to right in the order given"""
    order = by_cell(rows, cols)
    rows, cols, t = rows[order], cols[order], t[order]
    new = np.ones(rows.size, dtype=bool)
    new[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    starts = np.flatnonzero(new)
    run = np.cumsum(new) - 1
    rank = np.arange(rows.size) - starts[run] if rows.size else np.zeros(0, dtype=np.int64)
    acc = t[starts].copy()                          # the first product as it is: a lone -0.0 stays -0.0
    later = np.flatnonzero(rank > 0)
    later = later[np.argsort(rank[later], kind="stable")]
    edges = np.flatnonzero(np.diff(rank[later], prepend=0, append=np.iinfo(np.int64).max)) if later.size else []
    with np.errstate(all="ignore"):
        for lo, hi in zip(edges[:-1], edges[1:]):   # all products of one rank at once: a run has each rank once
            sel = later[lo:hi]
            acc[run[sel]] = acc[run[sel]] + t[sel]
    indptr = np.zeros(m + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(rows[starts], minlength=m))
    return indptr, cols[starts].astype(np.int32), acc


def spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n):
    """(indptr, indices, values) of A B for the CSR arrays of an m x K A and a K x n B"""
    rows, cols, t = expand(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    return fold(rows, cols, t, np.asarray(Ap).size - 1)


def products(Ap, Aj, Bp, K):
    """how many products the count pass reports: the B-row lengths over A's entries with a column inside [0, K)"""
    Aj, Bp = np.asarray(Aj, dtype=np.int64), np.asarray(Bp, dtype=np.int64)
    k = Aj[(Aj >= 0) & (Aj < K)]
    return int((Bp[k + 1] - Bp[k]).sum())


def row_bounds(Ap, Aj, Bp, K, n):
    """ub_i = min(f_i, n) per row, f_i the number of products of row i"""
    Ap, Aj, Bp = (np.asarray(a, dtype=np.int64) for a in (Ap, Aj, Bp))
    ok = (Aj >= 0) & (Aj < K)
    lens = np.where(ok, Bp[np.where(ok, Aj, 0) + 1] - Bp[np.where(ok, Aj, 0)], 0) if Bp.size > 1 else np.zeros(Aj.size, np.int64)
    f = np.add.reduceat(np.concatenate([lens, [0]]), Ap[:-1])
    f[Ap[:-1] == Ap[1:]] = 0
    return np.minimum(f, n)


def abs_sums(Ap, Aj, Ax, Bp, Bj, Bx, K, n):
    """(sum of |product|, number of products) per stored cell of the result, in the result's order: what the any-order
    bound len * 2^-53 * sum|a b| of a cell is made of"""
    rows, cols, t = expand(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    order = by_cell(rows, cols)
    rows, cols, t = rows[order], cols[order], np.abs(t[order])
    new = np.ones(rows.size, dtype=bool)
    new[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    starts = np.flatnonzero(new)
    return np.add.reduceat(t, starts) if starts.size else np.zeros(0), np.diff(np.append(starts, rows.size))


def to_dense(indptr, indices, values, n):
    m = indptr.size - 1
    out = np.zeros((m, n))
    np.add.at(out, (np.repeat(np.arange(m), np.diff(indptr)), indices), values)
    return out
