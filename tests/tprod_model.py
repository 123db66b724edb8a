"""CPU model of the transposed products (include/mxgpu_tprod.h): the terms of a segmented dot product, the operands of
its test cases and the pattern cases of tests/test_gpu_tprod.py.  The sums themselves are reduce_model's: a segmented dot
is the segmented sum of its written-out products, and numpy's f64 product is the same correctly rounded product the
kernel forms, so reduce_model.segment_reduce over the terms, with its any-order bound, is the oracle."""
import numpy as np

import reduce_model as RM


def terms(x, perm, key, w):
    """t[q] = x[perm[q]] * w[key[q]] in segment order (x None: every entry is 1)"""
    wk = np.asarray(w, dtype=np.float64)[np.asarray(key, dtype=np.int64)]
    if x is None:
        return wk
    xs = np.asarray(x, dtype=np.float64)
    xs = xs if perm is None else xs[np.asarray(perm, dtype=np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        return xs * wk


def in_storage_order(t, perm):
    """the products where mxd_segment_reduce with the same perm finds them: tx[perm[q]] = t[q]"""
    if perm is None:
        return t.copy()
    tx = np.empty_like(t)
    tx[np.asarray(perm, dtype=np.int64)] = t
    return tx


def rows_of_entries(p):
    p = np.asarray(p, dtype=np.int64)
    return np.repeat(np.arange(p.size - 1), np.diff(p)).astype(np.int32)


def _csr(m, rows, cols, seed):
    """the CSR pattern of the triplets in a shuffled order inside each row (rows unsorted), with the cell of the first
    triplet stored twice when there are two or more"""
    rows, cols = np.asarray(rows, dtype=np.int64).copy(), np.asarray(cols, dtype=np.int64).copy()
    if rows.size >= 2:
        rows[1], cols[1] = rows[0], cols[0]
    o = np.random.default_rng(seed).permutation(rows.size)
    rows, cols = rows[o], cols[o]
    o = np.argsort(rows, kind="stable")
    p = np.zeros(m + 1, dtype=np.int32)
    p[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return p, cols[o].astype(np.int32)


def _random(m, K, nnz, seed, lo=0, hi=None):
    rng = np.random.default_rng(seed)
    return _csr(m, rng.integers(0, m, size=nnz), rng.integers(lo, K if hi is None else hi, size=nnz), seed + 1)


def pattern_cases():
    """name -> (p, j, m, K): every pattern has unsorted rows and, from two entries on, a repeated (row, column)"""
    out = {"nnz-0": (np.zeros(8, dtype=np.int32), np.zeros(0, dtype=np.int32), 7, 5)}
    for nnz in (1, RM.TILE - 1, RM.TILE, RM.TILE + 1):
        out[f"nnz-{nnz}"] = _random(60, 9, nnz, nnz) + (60, 9)
    rng = np.random.default_rng(77)
    cols = np.concatenate([np.zeros(RM.TILE, dtype=np.int64), rng.integers(1, 3, size=1000)])
    out["column-ends-on-the-tile-edge"] = _csr(50, rng.integers(0, 50, size=cols.size), cols, 78) + (50, 3)
    out["empty-columns-and-rows-at-both-ends"] = _csr(
        200, rng.integers(20, 180, size=1500), rng.integers(5, 35, size=1500), 79) + (200, 40)
    out["one-column"] = _random(500, 1, 700, 80) + (500, 1)
    out["one-row"] = _random(1, 60, 200, 81) + (1, 60)
    m = 9000
    extra = int(0.02 * m * 39)
    out["9000x40-dense-first-column"] = _csr(
        m, np.concatenate([np.arange(m), rng.integers(0, m, size=extra)]),
        np.concatenate([np.zeros(m, dtype=np.int64), rng.integers(1, 40, size=extra)]), 82) + (m, 40)
    return out


def column_form(p, j, K):
    """(perm, key, segptr, nw) of X^T w: the column order, the entry rows in that order, the column pointer"""
    perm, colptr = RM.column_order(j, K)
    return perm, rows_of_entries(p)[perm], colptr, int(np.asarray(p).size - 1)


def row_form(p, j, K):
    """(perm, key, segptr, nw) of X w on the same scheme"""
    return None, np.asarray(j, dtype=np.int32), np.asarray(p, dtype=np.int32), int(K)


FLAVOURS = ("exact", "general", "special-x", "special-w", "pattern")
SPECIALS = [np.nan, np.inf, -0.0, -np.inf, np.nan, np.inf, -0.0]


def operands(name, nnz, nw, flavour, perm, key):
    """(x or None, w) of a case.  exact: integers in [-9, 9] in both; general: normal floats over six decades;
    special-x / special-w: the general ones with NaN, +Inf, -Inf and -0.0 where the entries at reduce_model's
    special positions (in segment order) read x, or w; pattern: no x."""
    rng = np.random.default_rng([len(name), nnz, nw, len(flavour)])
    nw = max(nw, 1)
    if flavour == "exact":
        return rng.integers(-9, 10, size=nnz).astype(np.float64), rng.integers(-9, 10, size=nw).astype(np.float64)
    w = rng.normal(size=nw) * 10.0 ** rng.integers(-3, 4, size=nw)
    if flavour == "pattern":
        return None, w
    x = rng.normal(size=nnz) * 10.0 ** rng.integers(-3, 4, size=nnz)
    at = RM.special_positions(nnz)
    if flavour == "special-x":
        for q, s in zip(at, SPECIALS):
            x[q if perm is None else perm[q]] = s
    if flavour == "special-w":
        for q, s in reversed(list(zip(at[::2], SPECIALS))):             # keys may repeat: the NaN is written last
            w[key[q]] = s
    return x, w
