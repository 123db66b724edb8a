"""The one-triangle sparse x sparse product at device level (include/mxgpu_gram.h): mxd_csr_spgemm_tri_count + _fill on
guarded buffers (tests/devmem.py), in the idiom of tests/test_gpu_spgemm.py, whose pattern builders it takes.  Outputs
and the workspace start as poison, the operands are checked untouched, the fill must not change out_indptr, every call
is made twice and must give the same bits.  The expectation is tests/gram_model.py (SM.expand, the keep rule, SM.fold):
pattern and values are compared bit for bit, NaN by class; the product count is the model's for each b_sorted.  Every
pattern runs with b_sorted = 0 as it is and with b_sorted = 1 on B with its rows sorted.  The bin edges come from
mxd_csr_spgemm_limits, so the cases sit on them whatever they are."""
import ctypes as C
import functools

import numpy as np
import pytest

import gram_model as GM
import spgemm_model as SM
from devmem import SLACK, GCsr, GuardedVec, _sync, value_dtype_of
from matrixextra_amd import _lib
from matrixextra_amd._lib import check
from test_gpu_spgemm import GU, KINDS, LU, bits, csr, full, limits, patterns, values_for

pytestmark = pytest.mark.gpu
U, L = _lib.MX_UPLO_UPPER, _lib.MX_UPLO_LOWER
assert (U, L) == (GM.UPPER, GM.LOWER)
MASKS = [(U, 0), (U, 1), (L, 0), (L, 1)]                                # (uplo, b_sorted)
mask_id = lambda ub: "UL"[ub[0]] + ("-sorted" if ub[1] else "-as-is")     # noqa: E731


def dev_spgemm_tri(Ap, Aj, Ax, Bp, Bj, Bx, K, n, uplo, b_sorted):
    """count + fill: (indptr, indices, values, products)"""
    lib = _lib.load()
    m = Ap.size - 1
    A, B = GCsr(Ap, Aj, Ax), GCsr(Bp, Bj, Bx)
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_spgemm_workspace_bytes(m, n))
    gp = GuardedVec(np.int32, n=m + 1)
    products, total = C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_csr_spgemm_tri_count(m, K, n, A.p.ptr, A.j.ptr, A.nnz, B.p.ptr, B.j.ptr, B.nnz, uplo, b_sorted, gp.ptr,
                                       gws.ptr, C.byref(products), C.byref(total), None))
    indptr = gp.result()                                                # every cell written
    gws._download()                                                     # the guards around the workspace
    nout = int(total.value)
    assert nout == indptr[m]
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(np.float64, n=nout + SLACK)
    check(lib.mxd_csr_spgemm_tri_fill(m, K, n, A.p.ptr, A.j.ptr, A.xptr, value_dtype_of(Ax), B.p.ptr, B.j.ptr, B.xptr,
                                      value_dtype_of(Bx), uplo, b_sorted, gp.ptr, gj.ptr, gx.ptr, gws.ptr, None))
    _sync()
    A.assert_untouched()
    B.assert_untouched()
    gws._download()
    assert np.array_equal(gp.result(), indptr), "the fill pass changed out_indptr"
    return indptr, gj.result(nout), gx.result(nout), int(products.value)


def run_and_compare(args, uplo, b_sorted, want=None, nan_by_class=False):
    """both passes, twice, against the model; `want` where the model's answer is shared between calls"""
    Ap, Aj, Ax, Bp, Bj, Bx, K, n = args
    wp, wj, wx = GM.spgemm_tri(*args, uplo) if want is None else want
    got = dev_spgemm_tri(*args, uplo, b_sorted)
    again = dev_spgemm_tri(*args, uplo, b_sorted)
    for a, b in zip(got[:3], again[:3]):                                # a repeated call: the same bits
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    p, j, x, products = got
    assert products == again[3] == GM.products(Ap, Aj, Bp, Bj, K, uplo, b_sorted)
    assert np.array_equal(p, wp) and np.array_equal(j, wj)
    if nan_by_class:
        nan = np.isnan(wx)
        assert np.array_equal(np.isnan(x), nan) and np.array_equal(bits(x[~nan]), bits(wx[~nan]))
    else:
        assert np.array_equal(bits(x), bits(wx))
    rows = np.repeat(np.arange(p.size - 1), np.diff(p))
    assert np.all(j >= rows) if uplo == U else np.all(j <= rows)        # nothing outside the triangle
    for r in range(p.size - 1):
        assert np.all(np.diff(j[p[r]:p[r + 1]]) > 0)                    # rows sorted, columns unique
    return p, j, x


def sorted_b(Bp, Bj):
    """B with every row ascending"""
    return Bp, GM.sort_rows(Bp, Bj, None)[1].astype(np.int32)


@functools.lru_cache(maxsize=None)
def pattern(name, b_sorted):
    """(Ap, Aj, Bp, Bj, K, n) of a pattern of tests/test_gpu_spgemm.py: as it is, or for b_sorted = 1 with B's rows sorted"""
    Ap, Aj, Bp, Bj, K, n = patterns()[name]
    return (Ap, Aj, *(sorted_b(Bp, Bj) if b_sorted else (Bp, Bj)), K, n)


@functools.lru_cache(maxsize=None)
def case(name, b_sorted, flavour):
    """the operands and the model's answers for both triangles, from one expansion"""
    Ap, Aj, Bp, Bj, K, n = pattern(name, b_sorted)
    Ax, Bx = values_for(name, flavour, "A", Aj.size), values_for(name, flavour, "B", Bj.size)
    args = (Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    rows, cols, t = SM.expand(*args)
    want = {}
    for uplo in (U, L):
        k = GM.keep(uplo, rows, cols)
        want[uplo] = SM.fold(rows[k], cols[k], t[k], Ap.size - 1)
    return args, want


# ---- the patterns of the unmasked product -------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
@pytest.mark.parametrize("name", sorted(patterns()))
def test_every_pattern_under_the_mask(gpu, name, mask):
    uplo, b_sorted = mask
    args, want = case(name, b_sorted, "general")
    p, j, x = run_and_compare(args, uplo, b_sorted, want[uplo])
    if name == "all_bins_mixed":                                        # the triangle of the whole product, bit for bit
        tp, tj, tx = GM.triangle_of(*SM.spgemm(*args), uplo)
        assert np.array_equal(p, tp) and np.array_equal(j, tj) and np.array_equal(bits(x), bits(tx))


def test_what_the_mask_leaves_of_the_patterns():
    """most patterns are rectangular: tall ones have rows without a window.  The congruent columns keep colliding under
    the upper mask (their rows are the first four); the lower mask leaves those rows nothing, which is a case too."""
    P = patterns()
    assert sum(Ap.size - 1 > n for Ap, Aj, Bp, Bj, K, n in P.values()) >= 2
    Ap, Aj, Bp, Bj, K, n = P["one_column"]
    assert GM.window(U, Ap.size - 1, n).tolist() == [1, 0, 0, 0]
    for name, slots in (("congruent_columns", 64), ("congruent_columns_block", 256)):
        p, j, _ = case(name, 0, "general")[1][U]
        first = j[p[0]:p[1]]
        assert first.size >= 20 and np.unique(first % slots).size == 1
        assert case(name, 0, "general")[1][L][1].size == 0
    mixed = {uplo: GM.row_bounds(*pattern("all_bins_mixed", 1)[:4], *P["all_bins_mixed"][4:], uplo, 1) for uplo in (U, L)}
    for ub in mixed.values():                                           # rows without a bin, lane groups, workgroups
        assert (ub == 0).any() and ((ub > 0) & (ub <= GU)).any() and ((ub > GU) & (ub <= LU)).any()
    # it has fewer rows than lds_ub, so the lower window keeps every row out of the dense bin: the staircase and
    # test_more_dense_rows_than_groups_under_the_mask have the dense rows of the lower mask
    assert (mixed[U] > LU).any() and not (mixed[L] > LU).any()


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
@pytest.mark.parametrize("name", sorted(patterns()))
def test_special_values_under_the_mask(gpu, name, mask):
    """NaN, +-Inf, -0.0 and 0.0 in either operand: NaN positions by class, everything else by bits"""
    uplo, b_sorted = mask
    args, want = case(name, b_sorted, "special")
    if name == "all_bins_mixed":
        assert np.isnan(want[uplo][2]).any() and np.isinf(want[uplo][2]).any() and (want[uplo][2] == 0).any()
    run_and_compare(args, uplo, b_sorted, want[uplo], nan_by_class=True)


@pytest.mark.parametrize("kinds", ["dd", "ln", "nn"])
@pytest.mark.parametrize("name", sorted(patterns()))
def test_value_kinds_under_the_mask(gpu, name, kinds):
    """l is read as a double with NA_LOGICAL -> NA_real_ and a stored FALSE kept as 0; n reads every entry as 1"""
    for uplo, b_sorted in MASKS:
        Ap, Aj, Bp, Bj, K, n = pattern(name, b_sorted)
        rng = np.random.default_rng([78, sum(map(ord, name))])
        Ax, Bx = KINDS[kinds[0]](rng, Aj.size), KINDS[kinds[1]](rng, Bj.size)
        run_and_compare((Ap, Aj, Ax, Bp, Bj, Bx, K, n), uplo, b_sorted, nan_by_class=True)


# ---- the staircase: the window moves rows across both bin edges -----------------------------------------------------------
N_STAIR = LU + 40


@functools.lru_cache(maxsize=None)
def staircase(b_sorted):
    """m = n = lds_ub + 40; B has three full rows (shuffled, or ascending for b_sorted = 1); row i of A has one entry,
    a few rows have two: ub_i = w_i runs through every value from n down to 1 (upper) or from 1 up to n (lower)"""
    n = N_STAIR
    Brows = [np.arange(n) if b_sorted else full(n, 40 + k) for k in range(3)]
    Arows = [[i % 3] for i in range(n)]
    for i in (0, 5, GU - 1, GU, LU - 1, LU, n - GU - 1, n - GU, n - LU - 1, n - LU, n - 1):
        Arows[i] = [i % 3, (i + 1) % 3]
    return (*csr(Arows), *csr(Brows), 3, n)


def test_the_staircase_reaches_every_edge_bin_and_lane_width_under_the_mask():
    n = N_STAIR
    assert limits(n, n)[:2] == (GU, LU)
    for uplo in (U, L):
        widths = set()
        for b_sorted in (0, 1):
            Ap, Aj, Bp, Bj, K, _ = staircase(b_sorted)
            ub = GM.row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, b_sorted)
            assert np.array_equal(ub, GM.window(uplo, n, n))            # ub_i = w_i on every row
            assert {LU + 1, LU, GU + 1, GU, 1} <= set(ub.tolist())      # each edge value occurs
            group, block, dense = (ub > 0) & (ub <= GU), (ub > GU) & (ub <= LU), ub > LU
            assert group.sum() == GU and block.sum() == LU - GU and dense.sum() == 40
            # without the mask every non-empty row is a dense row: the window is what moves them
            assert (SM.row_bounds(Ap, Aj, Bp, K, n) > LU).all()
            mean = GM.mean_step(Ap, Aj, Bp, Bj, K, uplo, b_sorted)[group]
            widths |= {8 if v <= 8 else 16 if v <= 16 else 32 for v in mean.tolist()}
            if not b_sorted:
                assert widths == {32}                                   # untrimmed steps are n long
        assert widths == {8, 16, 32}                                    # the trimmed steps reach each lane width


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_staircase(gpu, mask):
    uplo, b_sorted = mask
    Ap, Aj, Bp, Bj, K, n = staircase(b_sorted)
    Ax, Bx = values_for("staircase", "general", "A", Aj.size), values_for("staircase", "general", "B", Bj.size)
    args = (Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    assert 1_000_000 < SM.products(Ap, Aj, Bp, K) < 1_300_000
    p, _, _ = run_and_compare(args, uplo, b_sorted)
    assert np.array_equal(np.diff(p), GM.window(uplo, n, n))            # every row fills its window


# ---- where the window falls in a sorted row of B --------------------------------------------------------------------------
def trim_case():
    """n = 12, 14 rows (the last two have no window under the upper mask).  B's rows are ascending: lengths 0 and 1, one
    that begins with negative columns and ends with columns >= n.  Most rows of A take every row of B; row 6 takes
    columns 0 and 1 alone and row 2 columns 9 .. 11 alone, so that one mask leaves them nothing."""
    n = 12
    Brows = [[], [5], [3, 4, 5, 8], [-7, -1, 0, 2, 6, 11, 12, 40], [0, 1], [9, 10, 11]]
    Arows = [list(range(6)) for _ in range(14)]
    Arows[6], Arows[2], Arows[12] = [4], [5], [4, 3]
    return (*csr(Arows), *csr(Brows), 6, n)


def test_trim_positions(gpu):
    Ap, Aj, Bp, Bj, K, n = trim_case()
    assert all(np.all(np.diff(Bj[Bp[k]:Bp[k + 1]]) > 0) for k in range(K))
    rng = np.random.default_rng(12)
    Ax, Bx = rng.normal(size=Aj.size), rng.normal(size=Bj.size)
    args = (Ap, Aj, Ax, Bp, Bj, Bx, K, n)
    got = {}
    for uplo, b_sorted in MASKS:
        got[uplo, b_sorted] = run_and_compare(args, uplo, b_sorted)
    for uplo in (U, L):                                                 # B is sorted: the same bits either way
        for a, b in zip(got[uplo, 0], got[uplo, 1]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    up, lo = np.diff(got[U, 1][0]), np.diff(got[L, 1][0])
    # the window starts before a row's first column (row 1, B row 2) and past its last one (row 9: a skipped step)
    row2 = Bj[Bp[2]:Bp[3]]
    assert (row2 >= 1).all() and not (row2 >= 9).any() and not (row2 <= 2).any() and (row2 <= 8).all()
    assert GM.products(Ap, Aj, Bp, Bj, K, U, 1) < GM.products(Ap, Aj, Bp, Bj, K, U, 0) == SM.products(Ap, Aj, Bp, K)
    # on a column equal to i the diagonal is kept by both masks: (5, 5) from B rows 1 and 2
    for uplo in (U, L):
        p, j, _ = got[uplo, 1]
        assert 5 in j[p[5]:p[6]].tolist()
    # a row all of whose products lie outside the triangle has a bin without the trim and ends with count 0
    ub0 = {uplo: GM.row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, 0) for uplo in (U, L)}
    ub1 = {uplo: GM.row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, 1) for uplo in (U, L)}
    assert ub0[U][6] == 2 and ub1[U][6] == 0 and up[6] == 0 and ub0[L][2] == 3 and ub1[L][2] == 0 and lo[2] == 0
    assert up[12] == up[13] == 0 and ub0[U][12] == 0 and lo[12] > 0     # no window at all under the upper mask
    # negative columns and columns >= n never reach the result, trimmed or not
    assert all(((j >= 0) & (j < n)).all() for _, j, _ in got.values())


def test_trim_positions_in_the_workgroup_bins(gpu):
    """the same in the staged kernels: two long ascending rows of B with columns outside [0, n) at both ends, rows of A
    whose window makes them lane-group, workgroup and dense rows"""
    n = LU + 40
    Brows = [np.concatenate([[-9, -3], np.arange(n), [n, n + 5, 2 ** 30]]),
             np.concatenate([[-1], np.arange(0, n, 2), [n + 1]])]
    at = sorted({0, 1, 5, GU - 1, GU + 3, LU - 3, LU + 2, n - LU - 3, n - LU + 2, n - GU - 3, n - GU + 1, n - 2, n - 1})
    Arows = [[0, 1] if i in at else [] for i in range(n)]
    Ap, Aj = csr(Arows)
    Bp, Bj = csr(Brows)
    rng = np.random.default_rng(13)
    args = (Ap, Aj, rng.normal(size=Aj.size), Bp, Bj, rng.normal(size=Bj.size), 2, n)
    for uplo in (U, L):
        ub = GM.row_bounds(Ap, Aj, Bp, Bj, 2, n, uplo, 1)[at]
        assert ((ub > 0) & (ub <= GU)).any() and ((ub > GU) & (ub <= LU)).any() and (ub > LU).any()
        a = run_and_compare(args, uplo, 0)
        b = run_and_compare(args, uplo, 1)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---- dense workgroups take their later rows on a clean accumulator -------------------------------------------------------
def dense_case(uplo, b_sorted):
    """more dense rows than dense workgroups under the mask: for the upper mask 24 rows against a wide result, for the
    lower one the rows behind lds_ub of a tall one; two entries on two full rows of B each"""
    m, n = (24, LU + 64) if uplo == U else (LU + 500, LU + 8)
    dg = limits(m, n)[2]
    first = 0 if uplo == U else LU
    rows = [[] for _ in range(m)]
    for r in range(first, min(m, first + dg + 40)):
        rows[r] = [0, 1] if r % 2 else [1, 0]
    B = [np.arange(n), np.arange(n)] if b_sorted else [full(n, 51), full(n, 52)]
    return (*csr(rows), *csr(B), 2, n), dg


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_more_dense_rows_than_groups_under_the_mask(gpu, mask):
    uplo, b_sorted = mask
    (Ap, Aj, Bp, Bj, K, n), dg = dense_case(uplo, b_sorted)
    ub = GM.row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, b_sorted)
    assert (ub > LU).sum() >= dg + 3                                    # a workgroup takes a second row
    rng = np.random.default_rng(14)
    run_and_compare((Ap, Aj, rng.normal(size=Aj.size), Bp, Bj, rng.normal(size=Bj.size), K, n), uplo, b_sorted)


# ---- cancelled sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_cancelled_sums_stay_as_explicit_zeros(gpu, mask):
    """pairs a b and -(a b) on one cell, in every kind of bin under the mask: the stored 0.0 is kept"""
    uplo, b_sorted = mask
    rng = np.random.default_rng(9)
    n = LU + 40
    Brows = [np.arange(n - 7, n) if uplo == U else np.arange(7), rng.permutation(n)[:GU + 20], rng.permutation(n)]
    if b_sorted:
        Brows = [np.sort(r) for r in Brows]
    Bvals = [rng.normal(size=r.size) for r in Brows]
    Bp, Bj = csr(Brows + Brows)                                         # rows 3 .. 5 repeat rows 0 .. 2
    Bx = np.concatenate(Bvals + Bvals)
    # the rows sit where the mask leaves them a wide window: at the top for the upper one, at the bottom for the lower
    Arows = [[] for _ in range(n)]
    Avals = [[] for _ in range(n)]
    first = 0 if uplo == U else n - 4
    for r, (cols, vals) in enumerate([([0, 3], [1.5, -1.5]), ([4, 1], [0.7, -0.7]), ([2, 5], [-3.0, 3.0]),
                                      ([0, 3, 3, 0], [2.0, -2.0, 2.0, -2.0])]):
        Arows[first + r], Avals[first + r] = cols, vals
    Ap, Aj = csr(Arows)
    Ax = np.concatenate([np.asarray(v, dtype=np.float64) for v in Avals])
    args = (Ap, Aj, Ax, Bp, Bj, Bx, 6, n)
    want = GM.spgemm_tri(*args, uplo)
    kept = np.diff(want[0])[first:first + 4]
    assert kept[0] == 7 == kept[3] and GU < kept[1] <= LU < kept[2]     # a lane group, a workgroup, a dense row
    assert want[2].size and not want[2].any() and not np.signbit(want[2]).any()
    run_and_compare(args, uplo, b_sorted, want)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_a_bad_uplo_and_negative_sizes_are_refused_before_any_launch(gpu):
    lib = _lib.load()
    err = lambda: lib.mx_last_error().decode()                          # noqa: E731
    F64 = _lib.MX_F64
    for bad in (2, -1, 85):                                             # no mx_uplo: refused with every pointer null
        assert lib.mxd_csr_spgemm_tri_count(1, 1, 1, None, None, 0, None, None, 0, bad, 0, None, None, None, None, None) != 0
        assert "uplo" in err()
        assert lib.mxd_csr_spgemm_tri_fill(1, 1, 1, None, None, None, F64, None, None, None, F64, bad, 1, None, None, None,
                                           None, None) != 0
        assert "uplo" in err()
    for dims in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert lib.mxd_csr_spgemm_tri_count(*dims, None, None, 0, None, None, 0, U, 1, None, None, None, None, None) != 0
        assert "negative dimension" in err()
        assert lib.mxd_csr_spgemm_tri_fill(*dims, None, None, None, F64, None, None, None, F64, L, 0, None, None, None, None,
                                           None) != 0
        assert "negative dimension" in err()
    assert lib.mxd_csr_spgemm_tri_count(1, 1, 1, None, None, -1, None, None, 0, U, 0, None, None, None, None, None) != 0
    assert "bad size" in err()
    assert lib.mxd_csr_spgemm_tri_count(1, 1, 1, None, None, 0, None, None, 0, U, 0, None, None, None, None, None) != 0
    assert "null pointer" in err()
    assert lib.mxd_csr_spgemm_tri_fill(1, 1, 1, None, None, None, _lib.MX_F32, None, None, None, F64, U, 0, None, None, None,
                                       None, None) != 0
    assert "unsupported value dtype" in err()
    assert lib.mxd_csr_spgemm_tri_fill(0, 1, 1, None, None, None, F64, None, None, None, F64, L, 1, None, None, None, None,
                                       None) == 0
