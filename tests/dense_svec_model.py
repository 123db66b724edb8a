"""numpy model of `matrix * sparseVector` (multiply_elemwise_dense_by_svec_template<>, src/operators.cpp:3699-4303) and of
the COO * dense gather (multiply_coo_by_dense<>, :721-770), with the fixture tests/golden/dense_svec_golden.npz that the
reference's own compiled code recorded.  Test infrastructure only.

The model restates the reference for VALID input (positions unique and inside 1..length; sorted on the CSR routes),
route by route, and carries the deviations that DESIGN.md §4.15 declares:
  1. route D: a cell index >= nrows * ncols is never written (the reference tests `>` and writes one cell past the
     matrix at index == nrows * ncols, :4273, :4290); `overruns` finds such input, and no fixture record may have it;
  2. route C, integer / logical X, keep_NAs: in the rows after the last stored position of each recycle segment the
     reference pushes (double)NA_INTEGER for an NA cell (:4113-4120) where its sibling loops push NA_real_; the model
     (and the device) hold NA_real_ there; `int_na_tail_cells` names those entries;
  5. route C, keep_NAs: the reference never rewinds its cursor into the vector (`curr_i`, set once at :4061), so from
     the second recycle segment on it finds no position stored and every row there goes through the loop of
     deviation 2.  The device recycles the vector there as it does without keep_NAs (row r is ruled by position
     r mod length); `recycles_under_keep` names the records, whose first segment is compared with the reference.
`model(..., as_reference=True)` restates the reference with 2 and 5 as it is, and is compared with the fixture in
every bit; `model(...)` is what the device computes.
Every value is a copy, a constant or one IEEE multiplication, so the comparison is bit for bit (`same`), NaN payloads
included, except where both factors of a product are NaN (`both_nan`: the surviving payload is the hardware's
choice), which may cover at most 5 % of a case."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_svec_golden.npz")

NA_INT = np.int32(-2147483648)
NA_REAL = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
C_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]       # C's NAN as the reference's compiler makes it

KINDS = ("numeric", "float32", "integer", "logical")
DTYPE = {"numeric": np.float64, "float32": np.float32, "integer": np.int32, "logical": np.int32}
SVEC_FN = {k: "multiply_elemwise_dense_by_svec_" + k for k in KINDS}
COO_FN = {"numeric": "multiply_coo_by_dense_numeric", "integer": "multiply_coo_by_dense_integer",
          "logical": "multiply_coo_by_dense_logical", "float32": "multiply_coo_by_dense_float32",
          "and": "logicaland_coo_by_dense_logical"}
KIND_OF_FN = {v: k for k, v in SVEC_FN.items()}
COO_KIND_OF_FN = {v: k for k, v in COO_FN.items()}


def route(nrows, ncols, length):
    """"A" / "D": dense result; "B" / "C": CSR result (:3720, :3765, :3984, :4235, in that order)."""
    if length == nrows * ncols:
        return "A"
    if length == nrows:
        return "B"
    if length < nrows and nrows % length == 0:
        return "C"
    return "D"


def special(X, kind):
    """The cells that keep_NAs writes where the vector does not cover them."""
    if kind in ("numeric", "float32"):
        return ~np.isfinite(X)
    return X == NA_INT


def fill_of(X, kind):
    """Their value: an f64 NaN unchanged, an f64 +-Inf and every float32 special as C's NAN, NA_INTEGER as NA_real_."""
    if kind == "numeric":
        return np.where(np.isnan(X), X, C_NAN)
    return np.full(X.shape, C_NAN if kind == "float32" else NA_REAL)


def product(X, val, kind, int_na=C_NAN, daxpy=False):
    """X * val per cell (val broadcasts), and whether both factors are NaN."""
    val = np.broadcast_to(np.asarray(val, dtype=np.float64), X.shape)
    with np.errstate(all="ignore"):
        if kind in ("numeric", "float32"):
            Xd = X.astype(np.float64)
            out = Xd * val
            if daxpy:                                      # :4012: y = 0 + alpha * x, and nothing at all for alpha == 0
                out = np.where(val == 0.0, 0.0, 0.0 + val * Xd)
                return out, np.isnan(Xd) & np.isnan(val)
            return out, np.isnan(Xd) & np.isnan(val)
        na = X == NA_INT
        out = np.where(na, int_na, X.astype(np.float64) * val)
        return out, np.zeros(X.shape, dtype=bool)


def recycles_under_keep(nrows, ncols, nnz, length, keep):
    """Deviation 5 applies: route C under keep_NAs with a stored position and more than one segment."""
    return bool(keep) and nnz > 0 and route(nrows, ncols, length) == "C"


def model(kind, X, ii, xx, length, keep, as_reference=False):
    """(result dict as the exports give it, both-NaN mask over X_dense in F order or over values)."""
    X = np.asfortranarray(X)
    ii, xx = np.asarray(ii, dtype=np.int64), np.asarray(xx, dtype=np.float64)
    nrows, ncols = X.shape
    F = nrows * ncols
    rt = route(nrows, ncols, length)
    pos = np.full(max(length, 1), -1, dtype=np.int64)
    if rt in "AD":
        pos[ii - 1] = np.arange(ii.size)                   # a repeated position: the last entry rules
        flat = X.reshape(-1, order="F")
        p = pos[np.arange(F) % max(length, 1)] if F else np.zeros(0, dtype=np.int64)
        out = np.zeros(F)
        if keep:
            out = np.where(special(flat, kind), fill_of(flat, kind), 0.0)
        st = p >= 0
        both = np.zeros(F, dtype=bool)
        if st.any():
            out[st], both[st] = product(flat[st], xx[p[st]], kind)
        return dict(X_dense=out.reshape((nrows, ncols), order="F")), both
    pos[ii[::-1] - 1] = np.arange(ii.size)[::-1]            # a repeated position: the first entry rules
    rp = pos[np.arange(nrows) % length]
    stored = rp >= 0
    if as_reference and rt == "C" and keep:                 # deviation 5: the cursor is used up after the first segment
        stored &= np.arange(nrows) < length
    sp = special(X, kind) & ~stored[:, None] if keep else np.zeros(X.shape, dtype=bool)
    take = sp | stored[:, None]
    indptr = np.zeros(nrows + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(take.sum(axis=1))
    rows, cols = np.nonzero(take)                           # row-major order: by row, columns ascending
    cell = X[rows, cols]
    values = fill_of(cell, kind)
    both = np.zeros(rows.size, dtype=bool)
    s = stored[rows]
    int_na = NA_REAL if (rt == "B" and not keep) else C_NAN                       # :3803 against :3897, :4040, :4145
    daxpy = rt == "C" and not keep and kind == "numeric"                          # :4005-4015
    values[s], both[s] = product(cell[s], xx[rp[rows[s]]], kind, int_na, daxpy)
    if as_reference and rt == "C" and keep and kind in ("integer", "logical"):    # deviation 2
        last = int(ii.max()) if ii.size else 0
        values[(~s) & ((rows >= length) | (rows >= last))] = -2147483648.0
    return dict(indptr=indptr, indices=cols.astype(np.int32), values=values), both


def overruns(nrows, ncols, ii, length):
    """Deviation 1: some position reaches cell index nrows * ncols exactly, on route D."""
    F = nrows * ncols
    if route(nrows, ncols, length) != "D" or length <= 0:
        return False
    t = np.asarray(ii, dtype=np.int64) - 1
    return bool(((t <= F) & ((F - t) % length == 0)).any())


def int_na_tail_cells(kind, X, ii, length, keep):
    """Deviation 2: the entries (a mask over the reference's CSR values) that it writes as (double)NA_INTEGER."""
    ref, _ = model(kind, X, ii, np.ones(np.asarray(ii).size), length, keep, as_reference=True)
    return None if "values" not in ref else ref["values"] == -2147483648.0


def coo_model(kind, X, ii, jj, xx):
    X = np.asarray(X)
    d = X[np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)]
    if kind == "and":
        a, b = np.asarray(xx, dtype=np.int32), d.astype(np.int32)
        out = np.where((a == NA_INT) & (b == NA_INT), NA_INT,
                       np.where(a == NA_INT, np.where(b != 0, NA_INT, 0),
                                np.where(b == NA_INT, np.where(a != 0, NA_INT, 0), (a != 0) & (b != 0))))
        return out.astype(np.int32), np.zeros(out.size, dtype=bool)
    xx = np.asarray(xx, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind in ("numeric", "float32"):
            dd = d.astype(np.float64)
            return xx * dd, np.isnan(xx) & np.isnan(dd)
        dd = (d != 0).astype(np.float64) if kind == "logical" else d.astype(np.float64)
        return np.where(d == NA_INT, NA_REAL, xx * dd), np.zeros(xx.size, dtype=bool)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(got, want, both, what, skip=None):
    """Bit for bit, NaN payloads included; NaN-ness alone where both factors were NaN (at most 5 % of the case)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    if got.dtype != np.float64:
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    g, w, both = got.reshape(-1, order="F"), want.reshape(-1, order="F"), np.asarray(both).reshape(-1)
    share = float(both.mean()) if both.size else 0.0
    assert share <= 0.05, f"{what}: the NaN * NaN exemption covers {share:.1%} of the case"
    gb, wb = bits(g).copy(), bits(w).copy()
    if both.any():
        assert np.isnan(g[both]).all() and np.isnan(w[both]).all(), what
        gb[both] = wb[both] = 0
    if skip is not None:
        gb[skip] = wb[skip] = 0
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, f"{what}: {bad.size} cells differ, first at {bad[0]}: {g[bad[0]]!r} ({gb[bad[0]]:#x}) != {w[bad[0]]!r} ({wb[bad[0]]:#x})"


def compare_results(got, want, both, what, skip=None):
    assert set(got) == set(want), f"{what}: {sorted(got)} != {sorted(want)}"
    if "X_dense" in want:
        assert got["X_dense"].flags.f_contiguous
        return same(got["X_dense"], want["X_dense"], both, what + "[X_dense]")
    same(got["indptr"], want["indptr"], None, what + "[indptr]")
    same(got["indices"], want["indices"], None, what + "[indices]")
    same(got["values"], want["values"], both, what + "[values]", skip=skip)


def compare_svec(fn, args, got, reference, what):
    """`got` (the device) for one dense * svec call whose reference result is `reference`: against model() in every
    bit, and against the reference in every bit apart from the named deviations: at the cells of 2 the reference must
    hold (double)NA_INTEGER and `got` NA_real_, and under 5 the rows of the first segment are compared and the
    reference must have found no stored row after it."""
    kind = KIND_OF_FN[fn]
    X, ii, xx, length, keep = np.asarray(args[0]), args[1], args[2], int(args[3]), bool(args[4])
    want, both = model(kind, X, ii, xx, length, keep)
    compare_results(got, want, both, what + " against the model")
    named = int_na_tail_cells(kind, X, ii, length, keep)
    if named is not None and named.any():
        assert keep and route(*X.shape, length) == "C" and kind in ("integer", "logical"), what
        assert np.all(reference["values"][named] == -2147483648.0), f"{what}: the reference no longer holds (double)NA_INTEGER"
    if not recycles_under_keep(*X.shape, np.asarray(ii).size, length, keep):
        if named is not None and named.any():
            assert np.all(bits(got["values"][named]) == bits(np.array([NA_REAL]))[0]), f"{what}: NA_real_ expected at the named cells"
        return compare_results(got, reference, both, what + " against the reference", skip=named)
    n = int(reference["indptr"][length])                    # the first segment: rows 0..length-1
    same(got["indptr"][:length + 1], reference["indptr"][:length + 1], None, what + "[indptr, first segment]")
    same(got["indices"][:n], reference["indices"][:n], None, what + "[indices, first segment]")
    same(got["values"][:n], reference["values"][:n], both[:n], what + "[values, first segment]", skip=named[:n])
    assert np.all(bits(got["values"][:n][named[:n]]) == bits(np.array([NA_REAL]))[0]), f"{what}: NA_real_ expected at the named cells"
    rows = np.repeat(np.arange(X.shape[0]), np.diff(reference["indptr"]))
    later = rows >= length
    assert special(X[rows[later], reference["indices"][later]], kind).all(), \
        f"{what}: the reference found a stored row after its first segment"


def compare_coo(rec_args, fn, got, want, what):
    kind = COO_KIND_OF_FN[fn]
    X, ii, jj, xx = rec_args
    _, both = coo_model(kind, X, ii, jj, xx)
    assert set(got) == set(want) == {"row", "col", "val"}, what
    same(got["row"], want["row"], None, what + "[row]")
    same(got["col"], want["col"], None, what + "[col]")
    same(got["val"], want["val"], both, what + "[val]")


# ----------------------------------------------------------------------------- seeded inputs shared by the generator and the tests
NROWS = (1, 63, 64, 65, 130)                    # the fill's tile is 64 x 64: below, at and above its edge, and two row tiles
NCOLS = (1, 2, 63, 64, 65)
PATTERNS = ("none", "one", "ends", "all", "some")
VALUES = np.array([2.0, -1.0, 0.0, 0.5, -3.0, np.nan, NA_REAL, np.inf, -np.inf, 0.1, -1.0, 0.0])


def lengths_for(nrows, ncols):
    """The lengths the issue names, each once, with the route it takes."""
    out = {}
    for L in (nrows * ncols, nrows, nrows // 2, nrows // 5, 7, nrows + 3):
        if L >= 1 and L not in out:
            out[L] = route(nrows, ncols, L)
    return sorted(out.items())


def make_X(kind, nrows, ncols, rng, clean=False):
    """Small values with zero cells, and special cells in every corner and on about 3 % of the rest."""
    base = rng.integers(-3, 4, size=(nrows, ncols))
    sp = rng.random((nrows, ncols)) < 0.03
    sp[0, 0] = sp[0, -1] = sp[-1, 0] = sp[-1, -1] = True
    if clean:
        sp[:] = False
    if kind == "numeric":
        X = np.asfortranarray(base * 0.1)
        pool = np.array([np.nan, NA_REAL, np.inf, -np.inf, np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]])
        X[sp] = pool[rng.integers(0, pool.size, size=int(sp.sum()))]
    elif kind == "float32":
        X = np.asfortranarray((base * 0.25).astype(np.float32))
        pool = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        X[sp] = pool[rng.integers(0, 3, size=int(sp.sum()))]
    else:
        X = np.asfortranarray((base != 0).astype(np.int32) if kind == "logical" else base.astype(np.int32))
        X[sp] = NA_INT
    return X


def make_vector(pattern, length, rng):
    if pattern == "none":
        ii = np.zeros(0, dtype=np.int64)
    elif pattern == "one":
        ii = np.array([length // 2 + 1])
    elif pattern == "ends":
        ii = np.unique([1, length])
    elif pattern == "all":
        ii = np.arange(1, length + 1)
    else:
        ii = np.unique(np.concatenate([[1, length], 1 + np.flatnonzero(rng.random(length) < 0.5)]))
    xx = VALUES[rng.integers(0, VALUES.size, size=ii.size)].copy()
    return ii.astype(np.int32), xx


def cells_of(nrows, ncols, ii, length):
    """For each stored entry, the flat column-major cells that it multiplies (a list of index arrays)."""
    rt = route(nrows, ncols, length)
    F = nrows * ncols
    out = []
    for t in np.asarray(ii, dtype=np.int64) - 1:
        if rt in "AD":
            out.append(np.arange(t, F, length))
        else:
            rows = np.arange(t, nrows, length)
            out.append((rows[:, None] + np.arange(ncols)[None, :] * nrows).reshape(-1))
    return out


def sanitise(kind, X, ii, xx, length, allow_both_nan=False):
    """Keeps the case inside what IEEE fixes: +-Inf never meets a zero (the sign of that NaN differs between hosts and
    the device) and, unless asked for, a NaN value never meets a NaN cell.  The offending VALUE becomes 2.0."""
    flat = np.asarray(X).reshape(-1, order="F")
    zero = flat == 0
    if kind in ("numeric", "float32"):
        inf, nan = np.isinf(flat), np.isnan(flat)
    else:
        inf = nan = np.zeros(flat.size, dtype=bool)
    xx = xx.copy()
    for k, cells in enumerate(cells_of(X.shape[0], X.shape[1], ii, length)):
        v = xx[k]
        if (np.isinf(v) and zero[cells].any()) or (v == 0 and inf[cells].any()) or \
                (np.isnan(v) and nan[cells].any() and not allow_both_nan):
            xx[k] = 2.0
    return xx


def svec_case(kind, nrows, ncols, length, pattern, seed, x_seed=None):
    """(X, ii, xx); X depends on x_seed alone when given, so that cases can share one matrix."""
    rng = np.random.default_rng(seed)
    X = make_X(kind, nrows, ncols, rng if x_seed is None else np.random.default_rng(x_seed))
    ii, xx = make_vector(pattern, length, rng)
    if route(nrows, ncols, length) == "D":                  # deviation 1: the position that the reference would write
        ok = (nrows * ncols - (ii.astype(np.int64) - 1)) % length != 0           # past the matrix stays out of every input
        ii, xx = ii[ok], xx[ok]
    return X, ii, sanitise(kind, X, ii, xx, length)


def coo_case(kind, nnz, seed, nrows=65, ncols=7):
    """(X, ii, jj, xx): triplets with repeats, NA cells in X (and NA logicals in xx for the and).  The triplets and
    the f64 values depend on (nnz, seed) only, so that the kinds share them."""
    rng = np.random.default_rng(seed)
    ii = rng.integers(0, nrows, size=nnz).astype(np.int32)
    jj = rng.integers(0, ncols, size=nnz).astype(np.int32)
    if nnz > 2:
        ii[-1], jj[-1] = ii[0], jj[0]
        ii[1], jj[1] = nrows - 1, ncols - 1
    xx = np.array([2.0, -1.0, 0.5, 3.0, np.nan, NA_REAL, -0.25])[rng.integers(0, 7, size=nnz)]
    dk = "logical" if kind == "and" else kind
    X = make_X(dk, nrows, ncols, np.random.default_rng(77000 + KINDS.index(dk)))      # one matrix a kind
    if dk in ("numeric", "float32"):
        X[np.isinf(X)] = 1.5                                # no Inf * 0 here either; NaN cells stay
        meet = np.isnan(xx) & np.isnan(X[ii, jj].astype(np.float64))
        xx[meet] = 2.0
    if kind == "and":
        xx = np.array([0, 1, NA_INT], dtype=np.int32)[rng.integers(0, 3, size=nnz)]
    return X, ii, jj, xx
