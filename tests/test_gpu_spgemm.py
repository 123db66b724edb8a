"""The sparse x sparse product at device level (include/mxgpu_spgemm.h): mxd_csr_spgemm_count + _fill on guarded
buffers (tests/devmem.py).  Outputs and the workspace start as poison, the operands are checked untouched, every call is
made twice and must give the same bits.  The expectation is tests/spgemm_model.py, which folds the products in the order
the header defines: pattern and values are compared bit for bit.  The bin edges come from mxd_csr_spgemm_limits, so the
cases sit on them whatever they are."""
import ctypes as C
import functools

import numpy as np
import pytest

import spgemm_model as SM
from conftest import csr_to_dense
from devmem import SLACK, Dev, GCsr, GuardedVec, _sync, value_dtype_of
from matrixextra_amd import _lib
from matrixextra_amd._lib import check

pytestmark = pytest.mark.gpu
NA = SM.NA_INT
i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                  # noqa: E731


def limits(m, n):
    g, l, d = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    check(_lib.load().mxd_csr_spgemm_limits(m, n, C.byref(g), C.byref(l), C.byref(d)))
    assert 0 < g.value < l.value and d.value >= 1
    return g.value, l.value, d.value


GU, LU, _ = limits(1, 1)


def csr(rows):
    """(indptr, indices) of a list of rows, each a sequence of column ids in storage order"""
    p = np.zeros(len(rows) + 1, dtype=np.int32)
    p[1:] = np.cumsum([len(r) for r in rows])
    return p, i32(np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)]))


def dev_spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n):
    """count + fill: (indptr, indices, values, products)"""
    lib = _lib.load()
    m = Ap.size - 1
    A, B = GCsr(Ap, Aj, Ax), GCsr(Bp, Bj, Bx)
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_spgemm_workspace_bytes(m, n))
    gp = GuardedVec(np.int32, n=m + 1)
    products, total = C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_csr_spgemm_count(m, K, n, A.p.ptr, A.j.ptr, A.nnz, B.p.ptr, B.j.ptr, B.nnz, gp.ptr, gws.ptr,
                                   C.byref(products), C.byref(total), None))
    indptr = gp.result()                                                # every cell written
    gws._download()                                                     # the guards around the workspace
    nout = int(total.value)
    assert nout == indptr[m]
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(np.float64, n=nout + SLACK)
    check(lib.mxd_csr_spgemm_fill(m, K, n, A.p.ptr, A.j.ptr, A.xptr, value_dtype_of(Ax), B.p.ptr, B.j.ptr, B.xptr,
                                  value_dtype_of(Bx), gp.ptr, gj.ptr, gx.ptr, gws.ptr, None))
    _sync()
    A.assert_untouched()
    B.assert_untouched()
    gws._download()
    assert np.array_equal(gp.result(), indptr), "the fill pass changed out_indptr"
    return indptr, gj.result(nout), gx.result(nout), int(products.value)


# ---- pattern cases: name -> (Ap, Aj, Bp, Bj, K, n) -------------------------------------------------------------------------
def full(n, seed=None):
    """all n columns, shuffled with a seed"""
    return np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)


def edge_case(edge, n):
    """single-entry rows whose bound is edge - 1, edge, edge + 1, and two-entry rows that reach the same bounds with
    overlapping rows of B"""
    half = edge // 2
    B = [full(edge - 1, 1), full(edge, 2), full(edge + 1, 3), np.arange(half), np.arange(half - 1, edge - 1),
         np.arange(half, edge + 1)]
    A = [[0], [1], [2], [3, 4], [3, 5], [4, 3], []]
    return (*csr(A), *csr(B), len(B), n)


@functools.lru_cache(maxsize=None)
def patterns():
    rng = np.random.default_rng(5)
    P = {}
    P["no_rows"] = (*csr([]), *csr([[0, 3], [1], [2]]), 3, 4)
    P["a_without_entries"] = (*csr([[], [], [], [], []]), *csr([[0, 3], [1], [2]]), 3, 4)
    P["b_without_entries"] = (*csr([[0, 2], [1], []]), *csr([[], [], []]), 3, 4)
    P["empty_rows_at_both_ends"] = (*csr([[], [], [1, 2], [3], [0], [], []]), *csr([[], [0, 5], [5, 1], [2], []]), 5, 6)
    P["one_inner_dimension"] = (*csr([[0], [], [0, 0], [0]]), *csr([[4, 0, 2]]), 1, 5)
    P["one_column"] = (*csr([[0, 2], [1], [], [2, 2, 0]]), *csr([[0], [], [0]]), 3, 1)
    P["one_row"] = (*csr([[3, 0, 1]]), *csr([[0, 1], [1, 2], [], [6, 0]]), 4, 7)
    P["around_group_ub"] = edge_case(GU, 2 * GU + 5)
    P["around_lds_ub"] = edge_case(LU, LU + 3)
    # f_i far above n: every product lands on few columns; the three sizes of n reach the three kinds of bin
    for name, n in (("many_products_few_columns_group", 5), ("many_products_few_columns_block", GU + 8),
                    ("many_products_few_columns_dense", LU + 3)):
        K = 50 if n <= LU else 6
        P[name] = (*csr([rng.permutation(K), rng.integers(0, K, size=2 * K)]), *csr([full(n, 10 + k) for k in range(K)]), K, n)
    # columns congruent modulo the table sizes, a large n and short rows: every key starts probing at one slot
    n = 2048 * 24
    P["congruent_columns"] = (*csr([[0], [1], [0, 1], [2]]),
                              *csr([5 + 64 * np.arange(20), 5 + 64 * np.arange(19, 29), 7 + 2048 * rng.permutation(24)]), 3, n)
    P["congruent_columns_block"] = (*csr([[0], [0, 1]]), *csr([9 + 256 * rng.permutation(100), 9 + 256 * np.arange(90, 120)]),
                                    2, 256 * 120)
    P["a_unsorted_with_repeats"] = (*csr([[4, 1, 4, 0, 1, 4], [2, 2], [3, 0, 3]]),
                                    *csr([[0, 1], [1, 2, 3], [0, 7], [7, 6, 5], [2, 0, 4]]), 5, 8)
    P["b_unsorted"] = (*csr([[0, 1, 2], [2, 0], [1]]), *csr([[5, 0, 3], [3, 9, 1, 0], [9, 8, 0, 5]]), 3, 10)
    # more dense rows than dense workgroups: two entries on two full rows of B each, so a workgroup takes its second and
    # third row on a cleared accumulator
    n, m = LU + 3, 24
    dg = limits(m, n)[2]
    assert dg + 3 <= m
    rows = [[0, 1] if r % 2 else [1, 0] for r in range(dg + 3)] + [[] for _ in range(m - dg - 3)]
    P["more_dense_rows_than_groups"] = (*csr([rows[i] for i in rng.permutation(m)]), *csr([full(n, 31), full(n, 32)]), 2, n)
    # every bin in one matrix, rows shuffled: B rows of 3 .. 2 LU entries, A rows of 0 .. 6 entries
    n, K = 3 * LU, 40
    lens = [3, 5, 8, 9, 15, 16, 17, 30, GU, GU + 1, 60, 100, LU // 2, LU, LU + 1, 2 * LU] * 3
    Brows = [np.sort(rng.choice(n, size=L, replace=False)) if k % 2 else rng.choice(n, size=L, replace=False)
             for k, L in enumerate(lens[:K])]
    small = [k for k in range(K) if lens[k] <= 9]
    Arows = [rng.choice(K, size=rng.integers(0, 7), replace=True) for _ in range(150)]
    Arows += [rng.choice(small, size=c, replace=True) for c in (1, 2, 3, 4) * 10]
    P["all_bins_mixed"] = (*csr([Arows[i] for i in rng.permutation(len(Arows))]), *csr(Brows), K, n)
    return P


def values_for(name, flavour, which, size):
    """the values of operand `which` ("A" / "B") of a case under a flavour"""
    rng = np.random.default_rng([sum(map(ord, name)), sum(map(ord, flavour)), ord(which)])
    if flavour == "exact":
        return rng.integers(-9, 10, size=size).astype(np.float64)
    x = rng.normal(size=size) * 10.0 ** rng.integers(-3, 4, size=size)  # six decades
    if flavour == "special":
        kind = rng.integers(0, 12, size=size)
        x = np.where(kind == 0, np.nan, np.where(kind == 1, np.inf, np.where(kind == 2, -np.inf,
                     np.where(kind == 3, -0.0, np.where(kind == 4, 0.0, x)))))
    return x


@functools.lru_cache(maxsize=None)
def case(name, flavour):
    Ap, Aj, Bp, Bj, K, n = patterns()[name]
    Ax, Bx = values_for(name, flavour, "A", Aj.size), values_for(name, flavour, "B", Bj.size)
    return (Ap, Aj, Ax, Bp, Bj, Bx, K, n), SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def run_and_compare(args, want, nan_by_class=False):
    Ap, Aj, Ax, Bp, Bj, Bx, K, n = args
    wp, wj, wx = want
    got = dev_spgemm(*args)
    again = dev_spgemm(*args)
    for a, b in zip(got[:3], again[:3]):                                # a repeated call: the same bits
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    p, j, x, products = got
    assert products == again[3] == SM.products(Ap, Aj, Bp, K)
    assert np.array_equal(p, wp) and np.array_equal(j, wj)
    if nan_by_class:
        nan = np.isnan(wx)
        assert np.array_equal(np.isnan(x), nan) and np.array_equal(bits(x[~nan]), bits(wx[~nan]))
    else:
        assert np.array_equal(bits(x), bits(wx))
    return p, j, x


def test_the_cases_reach_every_bin():
    P = patterns()
    ub = {name: SM.row_bounds(Ap, Aj, Bp, K, n) for name, (Ap, Aj, Bp, Bj, K, n) in P.items()}
    for edge, name in ((GU, "around_group_ub"), (LU, "around_lds_ub")):
        assert {edge - 1, edge, edge + 1} <= set(ub[name].tolist())
        assert P[name][5] > edge + 1
    assert P["around_lds_ub"][5] == LU + 3 and (LU + 3) % 32
    assert ub["many_products_few_columns_group"].max() <= GU < ub["many_products_few_columns_block"].max() <= LU
    assert ub["many_products_few_columns_dense"].min() > LU
    assert ub["congruent_columns"].max() <= GU < ub["congruent_columns_block"].min()
    dense_rows = int((ub["more_dense_rows_than_groups"] > LU).sum())
    assert dense_rows == limits(24, LU + 3)[2] + 3
    mixed = ub["all_bins_mixed"]
    assert (mixed == 0).any() and ((mixed > 0) & (mixed <= GU)).sum() > 20 and ((mixed > GU) & (mixed <= LU)).sum() > 20
    assert (mixed > LU).sum() > limits(mixed.size, P["all_bins_mixed"][5])[2] // 2
    Ap, Aj, Bp = P["all_bins_mixed"][:3]
    f = np.array([np.diff(Bp)[Aj[Ap[r]:Ap[r + 1]]].mean() if Ap[r + 1] > Ap[r] else 0 for r in range(Ap.size - 1)])
    group = (mixed > 0) & (mixed <= GU)
    assert (f[group] <= 8).any() and ((f[group] > 8) & (f[group] <= 16)).any() and (f[group] > 16).any()   # each lane width


@pytest.mark.parametrize("flavour", ["exact", "general"])
@pytest.mark.parametrize("name", sorted(patterns()))
def test_pattern_and_values(gpu, name, flavour):
    args, want = case(name, flavour)
    p, j, x = run_and_compare(args, want)
    for r in range(p.size - 1):
        assert np.all(np.diff(j[p[r]:p[r + 1]]) > 0)                    # rows sorted, columns unique
    if flavour == "exact":
        Ap, Aj, Ax, Bp, Bj, Bx, K, n = args
        assert np.array_equal(SM.to_dense(p, j, x, n), csr_to_dense(Ap, Aj, Ax, K) @ csr_to_dense(Bp, Bj, Bx, n))


EVERY_BIN = ["around_group_ub", "all_bins_mixed", "more_dense_rows_than_groups"]


@pytest.mark.parametrize("name", sorted(patterns()))
def test_special_values(gpu, name):
    """NaN, +-Inf, -0.0 and 0.0 in either operand: NaN positions by class, everything else by bits"""
    args, want = case(name, "special")
    if name in EVERY_BIN:                                               # they reach the result in every kind of bin
        assert np.isnan(want[2]).any() and np.isinf(want[2]).any() and (want[2] == 0).any()
    run_and_compare(args, want, nan_by_class=True)


def test_cancelled_sums_stay_as_explicit_zeros(gpu):
    """pairs a b and -(a b) on one cell, in every kind of bin: the stored 0.0 is kept, the pattern is the symbolic one"""
    rng = np.random.default_rng(9)
    n = LU + 40
    Brows = [np.arange(7), rng.permutation(GU + 20), rng.permutation(LU + 9)]
    Bvals = [rng.normal(size=r.size) for r in Brows]
    Bp, Bj = csr(Brows + Brows)                                         # rows 3 .. 5 repeat rows 0 .. 2
    Bx = np.concatenate(Bvals + Bvals)
    Ap, Aj = csr([[0, 3], [4, 1], [2, 5], [0, 3, 3, 0]])
    Ax = np.array([1.5, -1.5, 0.7, -0.7, -3.0, 3.0, 2.0, -2.0, 2.0, -2.0])
    want = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, 6, n)
    assert np.array_equal(np.diff(want[0]), [7, GU + 20, LU + 9, 7]) and not want[2].any() and not np.signbit(want[2]).any()
    run_and_compare((Ap, Aj, Ax, Bp, Bj, Bx, 6, n), want)
    Bx0 = Bx.copy()
    Bx0[::2] = 0.0                                                      # a product with a stored zero stays an entry
    want0 = SM.spgemm(Ap, Aj, np.abs(Ax), Bp, Bj, Bx0, 6, n)
    assert np.array_equal(want0[0], want[0]) and (want0[2] == 0).any()
    run_and_compare((Ap, Aj, np.abs(Ax), Bp, Bj, Bx0, 6, n), want0)


KINDS = {"d": lambda rng, k: rng.integers(-9, 10, size=k).astype(np.float64),
         "l": lambda rng, k: rng.choice(np.array([1, 1, 0, NA], dtype=np.int32), size=k), "n": lambda rng, k: None}


@pytest.mark.parametrize("kinds", ["dd", "ld", "nd", "dn", "nn", "ll"])
@pytest.mark.parametrize("name", sorted(patterns()))
def test_value_kinds(gpu, name, kinds):
    """l is read as a double with NA_LOGICAL -> NA_real_ and a stored FALSE kept as 0; n reads every entry as 1"""
    Ap, Aj, Bp, Bj, K, n = patterns()[name]
    rng = np.random.default_rng([77, sum(map(ord, name))])
    Ax, Bx = KINDS[kinds[0]](rng, Aj.size), KINDS[kinds[1]](rng, Bj.size)
    want = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    if "l" in kinds and name in EVERY_BIN:
        assert np.isnan(want[2]).any() and (want[2] == 0).any()
    p, j, x = run_and_compare((Ap, Aj, Ax, Bp, Bj, Bx, K, n), want, nan_by_class=True)
    if kinds == "nn":                                                   # the number of paths
        A1, B1 = csr_to_dense(Ap, Aj, np.ones(Aj.size), K), csr_to_dense(Bp, Bj, np.ones(Bj.size), n)
        assert np.array_equal(SM.to_dense(p, j, x, n), A1 @ B1)


def test_general_values_against_the_reference_product(gpu):
    """the reference's own CSR x dense product on B.toarray() (its daxpy may fuse and adds in another grouping): every
    stored cell within len * 2^-53 * sum|a b| of it, the any-order bound of a sum of len terms"""
    from oracle import oracle as O
    args, want = case("all_bins_mixed", "general")
    Ap, Aj, Ax, Bp, Bj, Bx, K, n = args
    p, j, x = run_and_compare(args, want)
    ref = O.tcrossprod_csr_dense_numeric(Ap, Aj, Ax, np.asfortranarray(csr_to_dense(Bp, Bj, Bx, n).T), 1)
    rows = np.repeat(np.arange(p.size - 1), np.diff(p))
    sums, lens = SM.abs_sums(*args)
    err = np.abs(x - ref[rows, j])
    assert np.all(err <= lens * 2.0 ** -53 * sums)
    stored = np.zeros(ref.shape, dtype=bool)
    stored[rows, j] = True
    assert not ref[~stored].any()


def test_indices_out_of_range_contribute_nothing(gpu):
    """an A column outside [0, K) contributes nothing and a B column outside [0, n) is skipped; both stay in bounds"""
    K, n = 4, LU + 50
    Brows = [[0, n, 3, -1], np.concatenate([np.arange(GU + 5), [n + 7, -3]]), np.concatenate([[2 ** 30], np.arange(LU + 20)]),
             [1, 2]]
    Bp, Bj = csr(Brows)
    Ap, Aj = csr([[0, K, 3], [-1, 1, 4, 0], [2, 2 ** 30, 2], [K, -5], [3, -2 ** 31, 3]])
    rng = np.random.default_rng(3)
    Ax, Bx = rng.integers(-9, 10, size=Aj.size).astype(np.float64), rng.integers(-9, 10, size=Bj.size).astype(np.float64)
    want = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    assert np.array_equal(np.diff(want[0]), [4, GU + 5, LU + 20, 0, 2])
    p, j, x = run_and_compare((Ap, Aj, Ax, Bp, Bj, Bx, K, n), want)
    keepA, keepB = (Aj >= 0) & (Aj < K), (Bj >= 0) & (Bj < n)
    A = csr_to_dense(Ap, np.where(keepA, Aj, 0), np.where(keepA, Ax, 0.0), K)
    B = csr_to_dense(Bp, np.where(keepB, Bj, 0), np.where(keepB, Bx, 0.0), n)
    assert np.array_equal(SM.to_dense(p, j, x, n), A @ B)


def test_a_result_beyond_int32_max_is_refused_by_the_count_pass(gpu):
    """pattern operands 46 341 x 1 and 1 x 46 341, all stored: 46 341^2 = 2 147 488 281 entries.  The count pass alone
    runs; it returns the error, which names INT32_MAX, and the product count."""
    lib = _lib.load()
    s = 46341
    Ap, Aj = Dev(np.arange(s + 1, dtype=np.int32)), Dev(np.zeros(s, dtype=np.int32))
    Bp, Bj = Dev(np.array([0, s], dtype=np.int32)), Dev(np.arange(s, dtype=np.int32))
    out_p = GuardedVec(np.int32, n=s + 1)
    ws = Dev(nbytes=lib.mxd_csr_spgemm_workspace_bytes(s, s))
    products, total = C.c_int64(-1), C.c_int64(-1)
    rc = lib.mxd_csr_spgemm_count(s, 1, s, Ap.ptr, Aj.ptr, s, Bp.ptr, Bj.ptr, s, out_p.ptr, ws.ptr, C.byref(products),
                                  C.byref(total), None)
    assert rc != 0 and "INT32_MAX" in lib.mx_last_error().decode()
    assert products.value == s * s == total.value and s * s > 2 ** 31 - 1
    out_p._download()                                                   # the guards
