"""CPU model of the reduction family (include/mxgpu_reduce.h): the segmented reduction, the column order of a CSR
pattern, the diagonal, and the margin functions and norms built on them.  Plain Python and numpy, written from the
definitions; the GPU tests compare the device with it, tests/test_reduce_host.py compares it with dense numpy.

How a sum is pinned
-------------------
Neither R nor Matrix's code is available, so nothing is pinned bit for bit to reference C++; the two derivable pins are:

Exact data.  With integer-valued data whose partial sums stay below 2^53 every partial sum of every summation order
is an integer that f64 represents, so every order gives the same f64 and the device must equal numpy's result with
`==`.  That covers SUM, ABS_SUM and SQ_SUM, and norm "F" (the exact sum, then one correctly rounded sqrt).  ABS_MAX,
the diagonal, the permutation and the column pointer involve no rounding at all and are always compared exactly.

General floats.  The exact value S of a segment of k terms x_1..x_k is taken from math.fsum, which returns S rounded
once: |fsum - S| <= u |S| with u = 2^-53.  Any summation order of k terms in f64 (any tree, additions of the exact
identity 0 included) performs k - 1 rounded additions on the path of each term, so the computed sum is
sum x_i (1 + t_i) with |t_i| <= gamma_{k-1} <= gamma_k, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of
Numerical Algorithms, §4.2).  Hence
    |device - fsum| <= gamma_k * sum |x_i| + u |S|,
which `bound` returns with fsum(|x|) and |fsum| standing for the two exact quantities (both are within a factor
1 + u of them, far inside the slack between gamma_{k-1} and gamma_k).  For SQ_SUM each square is rounded once before
it is added (one more factor 1 + d, |d| <= u) on the device and in the model alike, which gives gamma_{k+2} * sum x^2
for the difference of the two.  No case is exempt: a segment with a NaN or an infinity has an exact expected class
(NaN, +Inf, -Inf) instead of a bound.
"""
import math

import numpy as np

SUM, ABS_SUM, SQ_SUM, ABS_MAX = 0, 1, 2, 3
OPS = (SUM, ABS_SUM, SQ_SUM, ABS_MAX)
OP_NAMES = {SUM: "sum", ABS_SUM: "abs_sum", SQ_SUM: "sq_sum", ABS_MAX: "abs_max"}
NA_LOGICAL = -2147483648
U = 2.0 ** -53
TILE = 4096


def gamma(k):
    return k * U / (1.0 - k * U)


def as_f64(values, kind, nnz):
    """the entries as the reduction sees them: 'd' as they are, 'l' TRUE = 1 / FALSE = 0 / NA = NaN, 'n' all 1"""
    if kind == "n":
        return np.ones(nnz)
    v = np.asarray(values)
    if kind == "l":
        return np.where(v == NA_LOGICAL, np.nan, (v != 0).astype(np.float64))
    return v.astype(np.float64)


def _map(op, x):
    return x if op == SUM else x * x if op == SQ_SUM else np.abs(x)


def _exact_sum(t):
    """the correctly rounded sum of finite terms; IEEE's answer when a term is not finite"""
    if t.size and not np.isfinite(t).all():
        with np.errstate(invalid="ignore"):
            return float(np.sum(t))
    return math.fsum(t.tolist())


def segment_reduce(op, f, segptr, perm=None, na_rm=False):
    """(out f64[nseg], skipped int32[nseg], bound f64[nseg]) of op over f[perm[q]], q in [segptr[s], segptr[s + 1]):
    out from fsum (or the maximum), bound as derived in the module docstring (0 for ABS_MAX and for results that are
    not finite: those are exact)."""
    segptr = np.asarray(segptr, dtype=np.int64)
    nseg = segptr.size - 1
    out, skipped, bnd = np.zeros(max(nseg, 0)), np.zeros(max(nseg, 0), dtype=np.int32), np.zeros(max(nseg, 0))
    g = f if perm is None else f[np.asarray(perm, dtype=np.int64)]
    for s in np.flatnonzero(np.diff(segptr) > 0):       # a segment without entries keeps 0, 0 skipped, bound 0
        x = g[segptr[s]:segptr[s + 1]]
        if na_rm:
            keep = ~np.isnan(x)
            skipped[s] = x.size - int(keep.sum())
            x = x[keep]
        t = _map(op, x)
        if op == ABS_MAX:
            out[s] = np.nan if np.isnan(t).any() else (t.max() if t.size else 0.0)
            continue
        out[s] = _exact_sum(t)
        if np.isfinite(out[s]):
            k = t.size + (2 if op == SQ_SUM else 0)
            bnd[s] = gamma(k) * math.fsum(np.abs(t).tolist()) + U * abs(out[s])
    return out, skipped, bnd


def assert_reduced(got, got_skipped, want, want_skipped, bound, what=""):
    """the device's (out, skipped) against segment_reduce's: the class of every result that is not finite, the bound
    for the others (0: equal), the counts exactly"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at other segments"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
    err = np.abs(got[fin] - want[fin])
    bad = np.flatnonzero(err > bound[fin])
    assert bad.size == 0, (f"{what}: {bad.size} segment(s) outside the bound, first {got[fin][bad[0]]!r} vs "
                           f"{want[fin][bad[0]]!r} (bound {bound[fin][bad[0]]!r})")
    if got_skipped is not None:
        assert np.array_equal(got_skipped, want_skipped), f"{what}: skipped counts differ"


def column_order(j, n):
    """(perm, colptr): the stable sort of the entries by column"""
    j = np.asarray(j, dtype=np.int64)
    colptr = np.zeros(n + 1, dtype=np.int32)
    colptr[1:] = np.cumsum(np.bincount(j, minlength=n)[:n]) if j.size else 0
    return np.argsort(j, kind="stable").astype(np.int32), colptr


def diag(p, j, values, kind, m, n):
    """the first stored (k, k) of row k in storage order, 0 without one: f64 for 'd', int32 for 'l' (NA kept) / 'n'"""
    d = min(m, n)
    out = np.zeros(d, dtype=np.float64 if kind == "d" else np.int32)
    for k in range(d):
        hit = np.flatnonzero(np.asarray(j[p[k]:p[k + 1]]) == k)
        if hit.size:
            out[k] = 1 if kind == "n" else values[p[k] + hit[0]]
    return out


def margin(op, p, j, values, kind, m, n, over_rows, na_rm=False, mean=False):
    """(result, skipped, bound) per row or per column of the m x n CSR; mean divides by the cells of the row / column
    less the skipped ones (cells that are not stored are zeros, not NAs); the bound is divided with it and takes the
    division's own rounding, u |result|"""
    f = as_f64(values, kind, len(j))
    if over_rows:
        out, skipped, bnd = segment_reduce(op, f, p, None, na_rm)
        cells = n
    else:
        perm, colptr = column_order(j, n)
        out, skipped, bnd = segment_reduce(op, f, colptr, perm, na_rm)
        cells = m
    if mean:
        with np.errstate(invalid="ignore", divide="ignore"):
            div = (cells - skipped).astype(np.float64)
            out = out / div
            bnd = np.where(np.isfinite(out), bnd / np.where(div > 0, div, 1.0) + U * np.abs(out), 0.0)
    return out, skipped, bnd


NORM_KINDS = {"O": "O", "o": "O", "1": "O", "I": "I", "i": "I", "F": "F", "f": "F", "M": "M", "m": "M"}


def norm(p, j, values, kind, m, n, type_):
    """(value, bound) of norm(X, type) for the m x n CSR: the table of norm_csr (R/csr_linalg.R:13-31)"""
    t = NORM_KINDS[type_]
    if m == 0 or n == 0 or len(j) == 0:
        return 0.0, 0.0
    f = as_f64(values, kind, len(j))
    whole = np.array([0, len(j)])
    if t == "M":
        return float(segment_reduce(ABS_MAX, f, whole)[0][0]), 0.0
    if t == "F":
        out, _, bnd = segment_reduce(SQ_SUM, f, whole)
        r = math.sqrt(out[0]) if not np.isnan(out[0]) else np.nan
        # d sqrt(s) = ds / (2 sqrt(s)), plus the sqrt's own rounding
        b = (bnd[0] / (2.0 * r) + U * r) if np.isfinite(r) and r > 0 and bnd[0] > 0 else 0.0
        return float(r), float(b)
    out, _, bnd = margin(ABS_SUM, p, j, values, kind, m, n, over_rows=(t == "I"))
    if np.isnan(out).any():
        return float("nan"), 0.0
    return float(out.max()), float(bnd.max())


# ---- the cases of the segmented reduction: the smallest shapes at which a tiled one can go wrong --------------------
def _segptr(lengths):
    sp = np.zeros(len(lengths) + 1, dtype=np.int32)
    sp[1:] = np.cumsum(lengths)
    return sp


def segment_cases():
    """name -> segptr"""
    rng = np.random.default_rng(2020)
    few = np.zeros(5000, dtype=np.int64)
    np.add.at(few, rng.integers(0, 5000, size=37), 1)
    return {
        "no-segments": _segptr([]),
        "five-empty-segments": _segptr([0] * 5),
        "one-entry": _segptr([1]),
        "one-segment-4095": _segptr([4095]),
        "one-segment-4096": _segptr([4096]),
        "one-segment-4097": _segptr([4097]),
        "three-tile-segment-between-empties": _segptr([0, 3, 10000, 0, 0, 1, 4090, 7, 0]),
        "boundary-on-entry-4096": _segptr([1000, 3096, 50, 0, 7]),
        "3000-short-segments": _segptr(rng.integers(1, 4, size=3000)),
        "5000-segments-37-entries": _segptr(few),
    }


def special_positions(nnz):
    """where the special values go: around the first tile edge and in the middle of the second tile, as far as the
    entries reach"""
    return [q for q in (0, TILE - 1, TILE, TILE + 1, TILE + TILE // 2, TILE + TILE // 2 + 1, nnz - 1) if 0 <= q < nnz]


def case_values(name, nnz, flavour):
    """(values, kind) of a case.  exact: integers in [-9, 9]; general: normal floats over six decades; special: the
    general ones with NaN, +Inf, -Inf and -0.0 at special_positions; logical: TRUE / FALSE / NA; pattern: none"""
    rng = np.random.default_rng([len(name), nnz, len(flavour)])
    if flavour == "pattern":
        return None, "n"
    if flavour == "logical":
        v = rng.choice(np.array([0, 1, NA_LOGICAL], dtype=np.int32), size=nnz, p=[0.2, 0.6, 0.2])
        for q in special_positions(nnz)[::2]:
            v[q] = NA_LOGICAL
        return v, "l"
    if flavour == "exact":
        return rng.integers(-9, 10, size=nnz).astype(np.float64), "d"
    v = rng.normal(size=nnz) * 10.0 ** rng.integers(-3, 4, size=nnz)
    if flavour == "special":
        for q, s in zip(special_positions(nnz), [np.nan, np.inf, -0.0, -np.inf, np.nan, np.inf, -0.0]):
            v[q] = s
    return v, "d"


FLAVOURS = ("exact", "general", "special", "logical", "pattern")
