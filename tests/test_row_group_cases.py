"""The case generator of the row-group tests (tests/rowgroup_cases.py) and the CPU oracle at its shapes, without a
GPU: every case selects the lane-group width it was made for, holds the row lengths and wavefront windows it claims,
has sorted unique columns, and the oracle's result on it equals an independent dense-numpy (and, where it imports,
scipy) computation of the same operation."""
import numpy as np
import pytest

import rowgroup_cases as R
from oracle import oracle as O

try:
    import scipy.sparse as sp
except Exception:                     # pragma: no cover - scipy is optional
    sp = None

CASES = R.all_cases(scale=1)
HALF_CASES = R.all_cases(scale=2)
ids = lambda cs: [c.id() for c in cs]                                                          # noqa: E731
NA = R.NA_INT


def same_values(got, want, msg=""):
    """bit for bit, the sign of zero included; NaN compared as NaN-ness"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, msg
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg)
        u = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
        np.testing.assert_array_equal(got.view(u)[~nan], want.view(u)[~nan], err_msg=msg)
    else:
        np.testing.assert_array_equal(got, want, err_msg=msg)


def r_logical(which, a, b):
    """R's three-valued |, &, xor on int32 logicals"""
    an, bn = a == NA, b == NA
    at, bt = (a != 0) & ~an, (b != 0) & ~bn
    if which == "or":
        out = np.where(at | bt, 1, np.where(an | bn, NA, 0))
    elif which == "and":
        out = np.where((~an & ~at) | (~bn & ~bt), 0, np.where(an | bn, NA, 1))
    else:
        out = np.where(an | bn, NA, (at != bt).astype(np.int64))
    return out.astype(np.int32)


def dense_of(res, K, dtype=None):
    v = res.get("values")
    if v is None or (np.asarray(v).size == 0 and res["indices"].size):
        v = np.ones(res["indices"].size)
    return R.dense(res["indptr"], res["indices"], np.asarray(v, dtype=dtype) if dtype else v, K)


def rows_sorted_unique(p, j):
    d = np.diff(j.astype(np.int64))
    inner = np.ones(j.size, dtype=bool)
    inner[p[1:-1][p[1:-1] < j.size]] = False          # the first entry of a row has no left neighbour in its row
    return bool((d > 0)[inner[1:]].all())


# ---------------------------------------------------------------------------------------------------- the generator
def test_mirror_of_pick_group():
    assert [R.pick_group(a) for a in (0, 3.9, 4, 4.01, 8, 8.5, 16, 33, 64, 65, 400)] == [4, 4, 4, 8, 8, 16, 16, 64, 64, 64, 64]
    assert R.merge_group(10, 30, 20) == 8 and R.merge_group(10, 90, 20) == 16 and R.merge_group(10, -1, 20) == 32
    assert R.spmv_group(10, -1) == 32 and R.half_group(10, 160) == 8
    for G in R.LANE_GROUPS:
        b, ms = 256 // G, R.row_counts(G)
        assert ms[:5] == [1, b - 1, b, b + 1, 3 * b + 1] and 1000 <= ms[5] <= 9999
        assert G == 64 or ms[5] % (64 // G) != 0            # one row a wavefront at G = 64: every m is a multiple


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_case_selects_its_width(c):
    G, m = c.G, c.m
    assert R.spmv_group(m, c.nnz) == G                                   # SpMV, svec, dvec, sort, colrange, colmap
    assert R.pick_group(c.nnz / m) == G
    assert R.spmv_group(c.rows_take.size, int(c.lens[c.rows_take].sum())) == G      # the gather: from its output
    assert R.half_group(m, 2 * c.nnz) == G                               # cbind of A with a matrix of A's size
    assert c.nnz2 <= c.nnz
    if G >= 8:
        assert R.merge_group(m, c.nnz, c.nnz2) == G
    # index vectors: repeats, first row, last row, a reversed range; column picks with repeats
    rt = c.rows_take
    assert rt[0] == 0 and rt[1] == m - 1 and np.array_equal(rt[2:2 + m], np.arange(m - 1, -1, -1))
    assert np.unique(rt).size < rt.size and rt.min() == 0 and rt.max() == m - 1
    assert np.unique(c.cols_unsorted).size < c.cols_unsorted.size and (np.diff(c.cols_sorted) >= 0).all()
    assert (np.diff(c.cols_unsorted) < 0).any()
    (_, lo0, hi0), (_, lo1, hi1), (_, lo2, hi2) = c.colranges()
    assert not ((c.j >= lo0) & (c.j <= hi0)).any() and lo1 == hi1 and (lo2, hi2) == (0, c.K - 1)


@pytest.mark.parametrize("c", HALF_CASES, ids=ids(HALF_CASES))
def test_half_mean_case_selects_its_width(c):
    assert R.half_group(c.m, c.nnz) == c.G                               # reverse-columns
    assert rows_sorted_unique(c.p, c.j)


@pytest.mark.parametrize("c", CASES + HALF_CASES, ids=ids(CASES + HALF_CASES))
def test_case_structure(c):
    G, m, wave = c.G, c.m, 64 // c.G
    assert c.p[0] == 0 and c.p[-1] == c.nnz and c.p2[-1] == c.nnz2
    assert rows_sorted_unique(c.p, c.j) and rows_sorted_unique(c.p2, c.j2)
    assert c.nnz == 0 or (0 <= c.j.min() and c.j.max() < c.K)
    assert c.nnz2 == 0 or (0 <= c.j2.min() and c.j2.max() < c.K)
    la, lb = c.lens, c.lens2
    for name, (start, count) in c.blocks.items():
        if name in R.REQUIRED:
            assert la[start] == R.required_length(name, G), name
    if m >= 1000:
        assert set(c.blocks) == set(R.REQUIRED) | {"register_windows", "one_long_window"}
        assert m % wave != 0 or wave == 1
        assert la.max() >= 200
        s = c.blocks["G-1"][0]
        assert list(la[s:s + 4]) == [G - 1, G, G + 1, 0]                 # next to each other
    if "register_windows" in c.blocks:
        s, n = c.blocks["register_windows"]
        assert s % wave == 0 and n % wave == 0 and n >= wave
        assert (la[s:s + n] <= G).all() and (lb[s:s + n] <= G).all()
        assert ((la[s:s + n] == G) & (lb[s:s + n] == G)).any()           # exactly G in both operands
        kinds = set(c.overlap[s:s + n])
        assert {"identical", "disjoint", "first", "last", "below", "above"} <= kinds
        assert (la[s:s + n] == 0).any() and (lb[s:s + n] == 0).any()     # one operand's row empty, both ways
    if "one_long_window" in c.blocks:
        s, n = c.blocks["one_long_window"]
        assert s % wave == 0 and n == wave
        assert int(((la[s:s + n] > G) | (lb[s:s + n] > G)).sum()) == 1
    # the overlap patterns are what they say
    for r in range(min(m, 200)):
        a, b = set(c.j[c.p[r]:c.p[r + 1]].tolist()), set(c.j2[c.p2[r]:c.p2[r + 1]].tolist())
        kind = c.overlap[r]
        if kind == "identical":
            assert a == b
        elif kind == "disjoint":
            assert not (a & b) and len(a) == len(b)
        elif kind in ("first", "last"):
            assert a & b == {min(a) if kind == "first" else max(a)}
        elif kind == "below":
            assert b and max(b) < min(a)                                 # every lower bound in B is n
        elif kind == "above":
            assert b and min(b) > max(a)                                 # every lower bound in B is 0
        elif kind == "a_empty":
            assert not a and b
        else:
            assert not b
    # values: an integer-valued set, a general set with specials, R logicals with NA
    xi, xg, xl = (c.vals[k][0] for k in ("int", "gen", "lgl"))
    assert np.array_equal(xi, np.round(xi)) and np.abs(xi).max(initial=0) <= 3
    assert set(np.unique(xl).tolist()) <= {0, 1, int(NA)}
    if m >= 1000:
        assert np.isnan(xg).any() and np.isinf(xg).any() and (xg == 0).any() and (xl == NA).any()


# --------------------------------------------------------------------------------- the oracle against dense numpy
@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_oracle_merges_against_dense(c):
    K = c.K
    for vk in ("int", "gen"):
        xa, xb = c.vals[vk]
        (Da, Sa), (Db, Sb) = R.dense(c.p, c.j, xa, K), R.dense(c.p2, c.j2, xb, K)
        with np.errstate(all="ignore"):
            for sub in (False, True):
                o = O.add_csr_elemwise(c.p, c.p2, c.j, c.j2, xa, xb, sub)
                Do, So = dense_of(o, K)
                want = np.where(Sa & Sb, Da + (-Db if sub else Db), np.where(Sa, Da, -Db if sub else Db))
                assert np.array_equal(So, Sa | Sb) and rows_sorted_unique(o["indptr"], o["indices"])
                same_values(Do[So], want[So], f"{vk} sub={sub}")
            o = O.multiply_csr_elemwise(c.p, c.p2, c.j, c.j2, xa, xb)
            Do, So = dense_of(o, K)
            assert np.array_equal(So, Sa & Sb)
            same_values(Do[So], (Da * Db)[So], vk)
    if sp is not None:
        xa, xb = c.vals["int"]
        A, B = sp.csr_matrix((xa, c.j, c.p), shape=(c.m, K)), sp.csr_matrix((xb, c.j2, c.p2), shape=(c.m, K))
        o = O.add_csr_elemwise(c.p, c.p2, c.j, c.j2, xa, xb, False)
        assert np.array_equal(dense_of(o, K)[0], (A + B).toarray())
        o = O.multiply_csr_elemwise(c.p, c.p2, c.j, c.j2, xa, xb)
        assert np.array_equal(dense_of(o, K)[0], A.multiply(B).toarray())
    xa, xb = c.vals["lgl"]
    (Da, Sa), (Db, Sb) = R.dense(c.p, c.j, xa, K), R.dense(c.p2, c.j2, xb, K)
    for which, xor in (("or", False), ("xor", True)):
        o = O.logicalor_csr_elemwise(c.p, c.p2, c.j, c.j2, xa, xb, xor)
        Do, So = dense_of(o, K)
        want = np.where(Sa & Sb, r_logical(which, Da, Db), np.where(Sa, Da, Db))
        assert np.array_equal(So, Sa | Sb) and np.array_equal(Do[So], want[So])
    o = O.logicaland_csr_elemwise(c.p, c.p2, c.j, c.j2, xa, xb)
    Do, So = dense_of(o, K)
    assert np.array_equal(So, Sa & Sb) and np.array_equal(Do[So], r_logical("and", Da, Db)[So])


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_oracle_slices_and_binds_against_dense(c):
    K, rt = c.K, c.rows_take
    xg, xl = c.vals["gen"][0], c.vals["lgl"][0]
    D, S = R.dense(c.p, c.j, xg, K)
    o = O.copy_csr_rows_numeric(c.p, c.j, xg, rt)
    Do, So = dense_of(o, K)
    assert np.array_equal(So, S[rt]) and o["indptr"][-1] == c.lens[rt].sum()
    same_values(Do[So], D[rt][So])
    for name, lo, hi in c.colranges():
        o = O.copy_csr_rows_col_seq_numeric(c.p, c.j, xg, rt, np.array([lo, hi], dtype=np.int32), False)
        width = hi - lo + 1
        Do, So = dense_of(o, width)
        wantS = S[rt][:, lo:hi + 1] if lo < K else np.zeros((rt.size, width), bool)
        assert np.array_equal(So, wantS), name
        if wantS.any():
            same_values(Do[So], D[rt][:, lo:hi + 1][So], name)
    for cols in (c.cols_sorted, c.cols_unsorted):
        o = O.copy_csr_arbitrary_numeric(c.p, c.j, xg, rt, cols)
        Do, So = dense_of(o, cols.size)
        assert np.array_equal(So, S[rt][:, cols]) and rows_sorted_unique(o["indptr"], o["indices"])
        same_values(Do[So], D[rt][:, cols][So])
    # cbind of A with its row-reversed self, shifted by K columns
    rev = np.arange(c.m - 1, -1, -1)
    y = O.copy_csr_rows_logical(c.p, c.j, xl, rev) if c.nnz else dict(indptr=c.p, indices=c.j, values=xl)
    o = O.cbind_csr_logical(c.p, c.j, xl, y["indptr"], y["indices"] + K, y["values"])
    Dl, Sl = R.dense(c.p, c.j, xl, K)
    Do, So = dense_of(o, 2 * K)
    assert np.array_equal(So, np.hstack([Sl, Sl[rev]])) and np.array_equal(Do, np.hstack([Dl, Dl[rev]]))
    # the row sort gives the sorted matrix back
    js, perm = R.shuffled_rows(c)
    sj, sx = O.sort_sparse_indices(c.p, js, xg[perm])
    assert np.array_equal(sj, c.j)
    same_values(sx, xg)
    assert O.check_indices_are_sorted(c.p, c.j) and (O.check_indices_are_sorted(c.p, js) == rows_sorted_unique(c.p, js))


@pytest.mark.parametrize("c", HALF_CASES, ids=ids(HALF_CASES))
def test_oracle_reverse_columns_against_dense(c):
    xg = c.vals["gen"][0]
    D, S = R.dense(c.p, c.j, xg, c.K)
    j, x = c.j.copy(), xg.copy()
    O.reverse_columns_inplace(c.p, j, x, c.K)
    Do, So = R.dense(c.p, j, x, c.K)
    assert np.array_equal(So, S[:, ::-1]) and rows_sorted_unique(c.p, j)
    same_values(Do[So], D[:, ::-1][So])


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_oracle_vector_products_against_dense(c):
    K, m = c.K, c.m
    rng = np.random.default_rng([c.G, m, 77])
    xi = c.vals["int"][0]
    D, S = R.dense(c.p, c.j, xi, K)
    v = rng.integers(-4, 5, size=K)
    vna = v.astype(np.int32)
    vna[rng.integers(0, K, size=3)] = NA
    assert np.array_equal(O.matmul_csr_dvec_numeric(c.p, c.j, xi, v.astype(np.float64)), D @ v)
    assert np.array_equal(O.matmul_csr_dvec_float32(c.p, c.j, xi, v.astype(np.float32)), (D @ v).astype(np.float32))
    if sp is not None:
        assert np.array_equal(sp.csr_matrix((xi, c.j, c.p), shape=(m, K)) @ v.astype(np.float64), D @ v)
    hit = (S & (vna == NA)[None, :]).any(axis=1)
    for fn, vv in ((O.matmul_csr_dvec_integer, np.where(vna == NA, 0, vna)),
                   (O.matmul_csr_dvec_logical, ((vna != 0) & (vna != NA)).astype(np.int64))):
        got = fn(c.p, c.j, xi, vna)
        assert np.array_equal(np.isnan(got), hit) and np.array_equal(got[~hit], (D @ vv)[~hit])
        assert ((got[hit].view(np.uint64) & np.uint64(0xFFFFFFFF)) == 1954).all()      # NA_real_: low word 1954
    yi = np.sort(rng.choice(K, size=K // 2, replace=False)).astype(np.int32) + 1
    yv = rng.integers(-4, 5, size=yi.size).astype(np.float64)
    vd = np.zeros(K)
    vd[yi - 1] = yv
    assert np.array_equal(O.matmul_csr_svec_numeric(c.p, c.j, xi, yi, yv), D @ vd)
    # X * v and X / v with R's recycling: position (row + col * m) mod length
    xg = c.vals["gen"][0]
    rows = np.repeat(np.arange(m, dtype=np.int64), c.lens)
    for length in (m, m * K, 7):
        dv = rng.normal(size=length)
        dv[rng.integers(0, length, size=2)] = [0.0, np.inf]
        at = (rows + c.j.astype(np.int64) * m) % length
        with np.errstate(all="ignore"):
            same_values(O.multiply_csr_by_dvec_no_NAs_numeric(c.p, c.j, xg, dv, K, True, False, False, False, False, True),
                        xg * dv[at])
            same_values(O.multiply_csr_by_dvec_no_NAs_numeric(c.p, c.j, xg, dv, K, False, False, True, False, False, True),
                        xg / dv[at])
            same_values(O.multiply_csr_by_dvec_no_NAs_numeric(c.p, c.j, xg, dv, K, False, False, True, False, False, False),
                        dv[at] / xg)
