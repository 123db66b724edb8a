"""numpy restatement of multiply_csr_by_dvec_with_NAs, written from its rules: the row-ruled regime
(the vector's length divides the number of rows) and the flat regime (any other length).  Values at stored cells of
plain rows and of the flat regime come from the CPU restatement of multiply_csr_by_dvec_no_NAs_numeric; fills are bit
patterns.  Test infrastructure only."""
import numpy as np

from oracle import oracle as O

NA_BITS, NAN_BITS = 0x7FF00000000007A2, 0x7FF8000000000000
OTHER_NAN_BITS = 0x7FF8000000000123


def from_bits(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


NA_REAL, NAN, OTHER_NAN = from_bits(NA_BITS), from_bits(NAN_BITS), from_bits(OTHER_NAN_BITS)
OPS = ("*", "^", "/", "%%", "%/%")
DIV = ("/", "%%", "%/%")


def flags(op):
    return tuple(op == o for o in OPS)


def is_na(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return np.isnan(v) & ((v.view(np.uint64) & np.uint64(0xFFFFFFFF)) == np.uint64(1954))


def special(op, v):
    v = np.asarray(v, dtype=np.float64)
    s = np.isnan(v)
    if op != "*":
        s = s | (v == 0)
    if op == "^":
        s = s | (v < 0)
    if op == "*":
        s = s | np.isinf(v)
    return s


def _stored(p, j, x, v, ncols, op, lhs=True):
    if len(j) == 0:
        return np.zeros(0)
    return O.multiply_csr_by_dvec_no_NAs_numeric(p, j, x, v, ncols, *flags(op), lhs)


def _row_rule(op, val):
    """(filled, fill value, stored columns keep a value of their own) of a row ruled by val"""
    nan = bool(np.isnan(val))
    if op == "*":
        if nan:
            return True, (NA_REAL if is_na([val])[0] else NAN), False
        return (True, NAN, True) if np.isinf(val) else (False, None, False)
    if op == "^":
        if nan:
            return True, val, True
        return (True, (1.0 if val == 0 else np.inf), True) if val <= 0 else (False, None, False)
    if val == 0:
        return True, NAN, True
    return (True, val, False) if nan else (False, None, False)


def model(p, j, x, v, ncols, op, X_is_LHS=True):
    """dict(indptr, indices, values, fill: bool per entry (a cell that the route adds or overwrites with a fill),
    exempt: bool per entry (under * and /, whose values are compared bit for bit: a stored cell whose NaN the
    operation itself made, or both operands NaN, where only NaN-ness is comparable), alias: the input structure is
    returned)."""
    if op in ("^", "/", "%%") and not X_is_LHS:
        raise ValueError("Internal error. Please file an issue in GitHub.")
    p, j = np.asarray(p, dtype=np.int32), np.asarray(j, dtype=np.int32)
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    m, L, nnz = p.size - 1, v.size, j.size
    rows_of = np.repeat(np.arange(m), np.diff(p))
    d = v[(rows_of + j.astype(np.int64) * m) % L] if nnz else np.zeros(0)
    stored = _stored(p, j, x, v, ncols, op)
    # under ^ %% %/% every value is compared with equal_nan, so NaN-ness is all that is ever compared there
    exempt_stored = np.isnan(stored) & ~(np.isnan(x) ^ np.isnan(d)) & (op in ("*", "/"))
    if L <= m and m % L == 0:
        op_, oj, ox, ofill, oex = [0], [], [], [], []
        for r in range(m):
            s, e = p[r], p[r + 1]
            filled, fill, looks_up = _row_rule(op, v[r % L])
            if not filled:
                oj.append(j[s:e]); ox.append(stored[s:e])
                ofill.append(np.zeros(e - s, bool)); oex.append(exempt_stored[s:e])
            else:
                vals, isf, ex = np.full(ncols, fill), np.ones(ncols, bool), np.zeros(ncols, bool)
                if looks_up:
                    for k in range(s, e):                       # the last entry of a repeated column wins
                        vals[j[k]], isf[j[k]], ex[j[k]] = stored[k], False, exempt_stored[k]
                oj.append(np.arange(ncols, dtype=np.int32)); ox.append(vals); ofill.append(isf); oex.append(ex)
            op_.append(op_[-1] + oj[-1].size)
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
        return dict(indptr=np.array(op_, dtype=np.int32), indices=cat(oj, np.int32), values=cat(ox, np.float64),
                    fill=cat(ofill, bool), exempt=cat(oex, bool), alias=False)
    N = m * ncols
    assert L <= N
    sp = np.flatnonzero(special(op, v))
    flat = np.concatenate([np.arange(ix, N, L, dtype=np.int64) for ix in sp]) if sp.size else np.zeros(0, np.int64)
    src = np.concatenate([np.full(len(range(ix, N, L)), ix) for ix in sp]) if sp.size else np.zeros(0, np.int64)
    nr, nc = flat % m, flat // m
    have = set((rows_of.astype(np.int64) * ncols + j).tolist())
    new = np.array([int(r) * ncols + int(c) not in have for r, c in zip(nr, nc)], dtype=bool)
    n_cand = flat.size
    nr, nc, src = nr[new], nc[new], src[new]
    if nr.size == 0:
        vals = _stored(p, j, x, v, ncols, op, X_is_LHS)
        return dict(indptr=p, indices=j, values=vals, fill=np.zeros(nnz, bool), exempt=exempt_stored, alias=True,
                    candidates=n_cand, new=0)
    sv = v[src]
    fillv = np.full(nr.size, NA_REAL)
    fillv[(sv < 0) & (op == "^")] = np.inf
    fillv[(sv == 0) & (op == "^")] = 1.0
    fillv[is_na(sv) | ((sv == 0) & (op in DIV))] = NAN
    ar = np.concatenate([rows_of, nr])
    ac = np.concatenate([j.astype(np.int64), nc])
    order = np.lexsort((ac, ar))
    indptr = np.zeros(m + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(ar, minlength=m))
    return dict(indptr=indptr, indices=ac[order].astype(np.int32), values=np.concatenate([stored, fillv])[order],
                fill=np.concatenate([np.zeros(nnz, bool), np.ones(nr.size, bool)])[order],
                exempt=np.concatenate([exempt_stored, np.zeros(nr.size, bool)])[order], alias=False,
                candidates=n_cand, new=int(nr.size))


def compare(got, exp, op, cap=0.05):
    """The comparison of the GPU tests: structure exact, fills bit for bit, stored cells bit for bit under * and /,
    rtol 1e-13 under ^ %% %/% (the tolerance of the values-only route), NaN-ness alone where exempt; the exempt share
    must stay under `cap`.  Returns that share."""
    np.testing.assert_array_equal(np.asarray(got["indptr"]), exp["indptr"])
    np.testing.assert_array_equal(np.asarray(got["indices"]), exp["indices"])
    gv, ev = np.ascontiguousarray(got["values"], dtype=np.float64), np.ascontiguousarray(exp["values"])
    assert gv.shape == ev.shape
    gb, eb = gv.view(np.uint64), ev.view(np.uint64)
    fill, exempt = exp["fill"], exp["exempt"]
    bad = np.flatnonzero(fill & (gb != eb))
    assert bad.size == 0, f"{bad.size} fill cell(s) differ, first at {bad[0]}: {gb[bad[0]]:#x} != {eb[bad[0]]:#x}"
    assert np.array_equal(np.isnan(gv), np.isnan(ev))
    st = ~fill & ~exempt
    if op in ("*", "/"):
        bad = np.flatnonzero(st & (gb != eb))
        assert bad.size == 0, f"{bad.size} stored value(s) differ, first at {bad[0]}: {gv[bad[0]]!r} != {ev[bad[0]]!r}"
    else:
        np.testing.assert_allclose(gv[st], ev[st], rtol=1e-13, atol=0, equal_nan=True)
    share = float(exempt.sum()) / max(exempt.size, 1)
    assert share <= cap, f"the NaN-ness exemption covers {share:.1%} of the entries"
    return share


# ---- generators shared by the host and the GPU tests ------------------------------------------------------------
def make_csr(m, ncols, density, seed, empty_rows=(), full_rows=(), positive=False):
    """sorted CSR with finite non-zero values (positive ones for ^, whose fractional exponents make NaNs of the rest)"""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, ncols)) < density
    for r in full_rows:
        mask[r, :] = True
    for r in empty_rows:
        mask[r, :] = False
    p = np.zeros(m + 1, dtype=np.int32)
    p[1:] = np.cumsum(mask.sum(axis=1))
    j = np.nonzero(mask)[1].astype(np.int32)
    x = np.round(rng.uniform(0.25, 4.0, size=j.size), 3) * rng.choice([-1.0, 1.0], size=j.size)
    return p, j, np.abs(x) if positive else x


def pool(op):
    """the special values an operation reacts to, covering its fill classes"""
    if op == "*":
        return [NA_REAL, OTHER_NAN, np.inf, -np.inf]
    if op == "^":
        return [NA_REAL, 0.0, -1.0, OTHER_NAN, -2.5, -np.inf]
    return [NA_REAL, OTHER_NAN, 0.0, -0.0]


def make_vector(L, op, seed, at=(), share=0.3):
    """finite values (positive small integers and halves, so that ^ stays finite), with specials at the positions
    `at` and at a random `share` of the others"""
    rng = np.random.default_rng(seed)
    v = rng.choice([0.5, 1.0, 1.5, 2.0, 3.0], size=L) * (rng.choice([-1.0, 1.0], size=L) if op != "^" else 1.0)
    pl = pool(op)
    where = set(int(a) % L for a in at) | set(np.flatnonzero(rng.random(L) < share).tolist())
    for n, ix in enumerate(sorted(where)):
        v[ix] = pl[n % len(pl)]
    return v


def dirty_case(op, flat):
    """X with NaN / Inf / 0 among its values, so that the operation itself makes NaNs (0/0, Inf*0, NaN op NaN)"""
    m, ncols = 40, 33
    p, j, x = make_csr(m, ncols, 0.5, 77)
    x = x.copy()
    x[::9] = 0.0
    x[4::9] = np.inf
    x[7::9] = NA_REAL
    x[2::31] = -np.inf
    L = 41 if flat else 20
    v = make_vector(L, op, 5, at=(0, L - 1), share=0.08)
    return p, j, x, v, ncols
