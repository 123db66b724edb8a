"""The row-group kernels (one G-lane group per row: spmv, merge, gather, sort, colslice, bind, svec, svecmul, dvec) at
every lane width G they are built for, the shared scan, and the grid-capped element kernels past their cap.

Every case comes from tests/rowgroup_cases.py: its true mean row length selects the intended G both at the device level
(the hint passed is the true nnz) and through the exports, and mxd_last_row_launch must report that G.  Operands sit
in sentinel-guarded device buffers (devmem.GuardedVec), outputs start as poison: a write outside [0, nnz_out), an
element left unwritten or a changed input fails the test.  The CPU oracle is the comparison; structure and copied or
single-operation values must match bit for bit (NaN as NaN-ness), sums within a bound derived from the operation count.
"""
import ctypes as C
import math

import numpy as np
import pytest

import rowgroup_cases as R
from devmem import (GCsr, GuardedVec, dev_by_dvec, dev_by_svec, dev_cbind, dev_colmap, dev_colrange, dev_gather,
                    dev_merge, dev_reverse_columns, dev_scan, dev_sort_rows, dev_spmv, dev_spmv_svec, last_row_launch)
from matrixextra_amd import _lib, exports as G
from matrixextra_amd._lib import MX_F32, MX_F64, MX_I32, MX_LGL, MX_NONE
from oracle import oracle as O
from test_row_group_cases import same_values

pytestmark = pytest.mark.gpu

CASES = R.all_cases(scale=1)
HALF_CASES = R.all_cases(scale=2)
MERGE_CASES = [c for c in CASES if c.G in R.MERGE_GROUPS]
ids = lambda cs: [c.id() for c in cs]                                                          # noqa: E731
NA = R.NA_INT
KINDS = ((MX_F64, "gen"), (MX_LGL, "lgl"), (MX_NONE, None))


def same_csr(got, want, msg=""):
    """(indptr, indices, values): structure bit-exact, values bit-exact with NaN as NaN-ness"""
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    if want[2] is not None and got[2] is not None:
        same_values(got[2], np.asarray(want[2]), msg)


def from_dict(d):
    v = d.get("values")
    return d["indptr"], d["indices"], (None if v is None or (np.asarray(v).size == 0 and d["indices"].size) else v)


def values_of(c, key, which=0):
    return None if key is None else c.vals[key][which]


# ------------------------------------------------------------------------------------------------------------- SpMV
def gamma_bound(row_len, G, u):
    """gamma_n with n = row length + log2(G) + 1: a row's products are added one by one by the lanes (at most
    row_len additions along any path), the butterfly adds log2(G) more, and one more rounding covers the product
    (fused or rounded).  Derived from the kernel's operation count, not measured."""
    n = row_len + int(math.log2(G)) + 1
    return n * u / (1.0 - n * u)


def check_sums(got, c, x, v_f64, G, u, msg):
    """|got - ref| <= gamma_n * sum |a_k v_k| per row, ref = the exactly rounded sum of the f64 products"""
    for r in range(c.m):
        s, e = int(c.p[r]), int(c.p[r + 1])
        prods = x[s:e] * v_f64[c.j[s:e]]
        ref, mag = math.fsum(prods), math.fsum(np.abs(prods))
        err = abs(float(got[r]) - ref)
        bound = gamma_bound(e - s, G, u) * mag
        assert err <= bound, f"{msg} row {r} (length {e - s}): |got - ref| = {err:.3e} > {bound:.3e}"


def dvec_operands(c):
    rng = np.random.default_rng([c.G, c.m, 5])
    vi = rng.integers(-4, 5, size=c.K).astype(np.int32)
    vna = vi.copy()
    vna[c.j[rng.integers(0, c.nnz, size=3)]] = NA           # columns that some row stores
    return vi, vna, rng.normal(size=c.K)


SPMV = ((MX_F64, np.float64, O.matmul_csr_dvec_numeric, G.matmul_csr_dvec_numeric),
        (MX_I32, np.int32, O.matmul_csr_dvec_integer, G.matmul_csr_dvec_integer),
        (MX_LGL, np.int32, O.matmul_csr_dvec_logical, G.matmul_csr_dvec_logical),
        (MX_F32, np.float32, O.matmul_csr_dvec_float32, G.matmul_csr_dvec_float32))


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_spmv(gpu, c):
    vi, vna, vg = dvec_operands(c)
    xi = c.vals["int"][0]
    xg = np.where(np.isfinite(c.vals["gen"][0]), c.vals["gen"][0], 1.5)
    Ai, Ag = GCsr(c.p, c.j, xi), GCsr(c.p, c.j, xg)
    for dt, npdt, oracle, export in SPMV:
        # integer-valued data: every summation order is exact
        v = (vna if dt in (MX_I32, MX_LGL) else vi).astype(npdt)
        want = oracle(c.p, c.j, xi, v)
        got, launch = dev_spmv(Ai, v, dt, c.nnz)
        assert launch == ("spmv", c.G)
        same_values(got, want, f"kind {dt}")
        if dt in (MX_I32, MX_LGL):
            na = np.isnan(want)
            assert na.any()
            assert ((got[na].view(np.uint64) & np.uint64(0xFFFFFFFF)) == 1954).all()       # NA_real_
        ex = export(c.p, c.j, xi, v)
        assert last_row_launch() == ("spmv", c.G)
        same_values(ex, want, f"export kind {dt}")
        # general data: the bound of gamma_bound
        v = (vi if dt in (MX_I32, MX_LGL) else vg).astype(npdt)
        vf = (v != 0).astype(np.float64) if dt == MX_LGL else v.astype(np.float64)
        got, launch = dev_spmv(Ag, v, dt, c.nnz)
        assert launch == ("spmv", c.G)
        check_sums(got, c, xg, vf, c.G, 2.0 ** -24 if dt == MX_F32 else 2.0 ** -53, f"kind {dt}")
        same_values(export(c.p, c.j, xg, v), got, "export and device level differ")


# ------------------------------------------------------------------------------------------------------------ merge
MERGES = ((_lib.MX_OP_ADD, ("int", "gen"), lambda *a: O.add_csr_elemwise(*a, False), lambda *a: G.add_csr_elemwise(*a, False)),
          (_lib.MX_OP_SUB, ("int", "gen"), lambda *a: O.add_csr_elemwise(*a, True), lambda *a: G.add_csr_elemwise(*a, True)),
          (_lib.MX_OP_MUL, ("int", "gen"), O.multiply_csr_elemwise, G.multiply_csr_elemwise),
          (_lib.MX_OP_OR, ("lgl",), lambda *a: O.logicalor_csr_elemwise(*a, False), lambda *a: G.logicalor_csr_elemwise(*a, False)),
          (_lib.MX_OP_XOR, ("lgl",), lambda *a: O.logicalor_csr_elemwise(*a, True), lambda *a: G.logicalor_csr_elemwise(*a, True)),
          (_lib.MX_OP_AND, ("lgl",), O.logicaland_csr_elemwise, G.logicaland_csr_elemwise))


@pytest.mark.parametrize("c", MERGE_CASES, ids=ids(MERGE_CASES))
def test_merge(gpu, c):
    ops = {}
    for vk in ("int", "gen", "lgl"):
        xa, xb = c.vals[vk]
        ops[vk] = (GCsr(c.p, c.j, xa), GCsr(c.p2, c.j2, xb))
    for op, value_sets, oracle, export in MERGES:
        for vk in value_sets:
            xa, xb = c.vals[vk]
            with np.errstate(all="ignore"):
                want = from_dict(oracle(c.p, c.p2, c.j, c.j2, xa, xb))
            A, B = ops[vk]
            p, j, x, total, launches = dev_merge(op, A, B, c.nnz, c.nnz2)
            assert launches == [("merge", c.G)] * 2
            assert total == want[1].size == p[-1]
            same_csr((p, j, x), want, f"op {op} {vk}")
            ex = from_dict(export(c.p, c.p2, c.j, c.j2, xa, xb))
            assert last_row_launch() == ("merge", c.G)
            same_csr(ex, want, f"export op {op} {vk}")


# ----------------------------------------------------------------------------------------------------------- gather
GATHER = {MX_F64: (O.copy_csr_rows_numeric, G.copy_csr_rows_numeric), MX_LGL: (O.copy_csr_rows_logical, G.copy_csr_rows_logical),
          MX_NONE: (O.copy_csr_rows_binary, G.copy_csr_rows_binary)}


def call_kind(fn, dt, p, j, x, *rest):
    return fn(p, j, *rest) if dt == MX_NONE else fn(p, j, x, *rest)


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_gather(gpu, c):
    rt = c.rows_take
    nout = int(c.lens[rt].sum())
    for dt, vk in KINDS:
        x = values_of(c, vk)
        want = from_dict(call_kind(GATHER[dt][0], dt, c.p, c.j, x, rt))
        p, j, xo, total, launch = dev_gather(GCsr(c.p, c.j, x), rt, dt, nout)
        assert launch == ("gather", c.G)
        assert total == nout == want[1].size
        same_csr((p, j, xo), want, f"dtype {dt}")
        ex = from_dict(call_kind(GATHER[dt][1], dt, c.p, c.j, x, rt))
        assert last_row_launch() == ("gather", c.G)
        same_csr(ex, want, f"export dtype {dt}")


# ---------------------------------------------------------------------------------------------------- column slices
COLSEQ = {MX_F64: (O.copy_csr_rows_col_seq_numeric, G.copy_csr_rows_col_seq_numeric),
          MX_LGL: (O.copy_csr_rows_col_seq_logical, G.copy_csr_rows_col_seq_logical),
          MX_NONE: (O.copy_csr_rows_col_seq_binary, G.copy_csr_rows_col_seq_binary)}
ARBITRARY = {MX_F64: (O.copy_csr_arbitrary_numeric, G.copy_csr_arbitrary_numeric),
             MX_LGL: (O.copy_csr_arbitrary_logical, G.copy_csr_arbitrary_logical),
             MX_NONE: (O.copy_csr_arbitrary_binary, G.copy_csr_arbitrary_binary)}


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_colrange(gpu, c):
    rt, avg = c.rows_take, c.nnz / c.m
    for dt, vk in KINDS:
        x = values_of(c, vk)
        A = GCsr(c.p, c.j, x)
        for name, lo, hi in c.colranges():
            cols = np.array([lo, hi], dtype=np.int32)
            want = from_dict(call_kind(COLSEQ[dt][0], dt, c.p, c.j, x, rt, cols, False))
            p, j, xo, total, launches = dev_colrange(A, rt, lo, hi, dt, avg)
            assert launches == [("mxd_csr_colrange_count", c.G), ("mxd_csr_colrange_fill", c.G)]
            assert total == want[1].size and (name != "empty" or total == 0) and (name != "all" or total == c.lens[rt].sum())
            same_csr((p, j, xo), want, f"{name} dtype {dt}")
            ex = from_dict(call_kind(COLSEQ[dt][1], dt, c.p, c.j, x, rt, cols, False))
            assert last_row_launch() == ("mxd_csr_colrange_fill" if total else "mxd_csr_colrange_count", c.G)
            same_csr(ex, want, f"export {name} dtype {dt}")


def sort_rows_host(p, j, x):
    """each row ordered by column id (ids are unique inside a row here)"""
    rows = np.repeat(np.arange(p.size - 1), np.diff(p))
    order = np.lexsort((j, rows))
    return p, j[order], None if x is None else x[order]


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_colmap(gpu, c):
    rt, avg = c.rows_take, c.nnz / c.m
    for dt, vk in KINDS:
        x = values_of(c, vk)
        A = GCsr(c.p, c.j, x)
        for cols, is_sorted in ((c.cols_sorted, True), (c.cols_unsorted, False)):
            want = from_dict(call_kind(ARBITRARY[dt][0], dt, c.p, c.j, x, rt, cols))
            p, j, xo, total, launches = dev_colmap(A, rt, cols, dt, avg)
            assert launches == [("mxd_csr_colmap_count", c.G), ("mxd_csr_colmap_fill", c.G)]
            assert total == want[1].size
            same_csr((p, j, xo) if is_sorted else sort_rows_host(p, j, xo), want, f"sorted={is_sorted} dtype {dt}")
            ex = from_dict(call_kind(ARBITRARY[dt][1], dt, c.p, c.j, x, rt, cols))
            # an unsorted selector ends with the row sort of the result, sized from the result's mean row length
            assert last_row_launch() == (("mxd_csr_colmap_fill", c.G) if is_sorted or total == 0
                                         else ("sort", R.spmv_group(rt.size, total)))
            same_csr(ex, want, f"export sorted={is_sorted} dtype {dt}")


# ------------------------------------------------------------------------------------------------------------ cbind
CBIND = {MX_F64: (O.cbind_csr_numeric, G.cbind_csr_numeric), MX_LGL: (O.cbind_csr_logical, G.cbind_csr_logical),
         MX_NONE: (O.cbind_csr_binary, G.cbind_csr_binary)}


def reversed_rows(c, x):
    """A with its rows in reverse order, columns shifted by K: the right-hand operand of the cbind"""
    lens = c.lens[::-1]
    p = np.zeros(c.m + 1, dtype=np.int32)
    p[1:] = np.cumsum(lens)
    take = np.concatenate([np.arange(c.p[r], c.p[r + 1]) for r in range(c.m - 1, -1, -1)]).astype(np.int64)
    return p, (c.j[take] + c.K).astype(np.int32), None if x is None else x[take]


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_cbind(gpu, c):
    for dt, vk in KINDS:
        x = values_of(c, vk)
        yp, yj, yx = reversed_rows(c, x)
        args = (c.p, c.j, yp, yj) if dt == MX_NONE else (c.p, c.j, x, yp, yj, yx)
        want = from_dict(CBIND[dt][0](*args))
        p, j, xo, launch = dev_cbind(GCsr(c.p, c.j, x), GCsr(yp, yj, yx), dt, 2 * c.nnz)
        assert launch == ("mxd_csr_cbind", c.G)
        same_csr((p, j, xo), want, f"dtype {dt}")
        ex = from_dict(CBIND[dt][1](*args))
        assert last_row_launch() == ("mxd_csr_cbind", c.G)
        same_csr(ex, want, f"export dtype {dt}")


# ------------------------------------------------------------------------------------------- sort / reverse-columns
@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_sort_rows(gpu, c):
    js, perm = R.shuffled_rows(c)
    for dt, vk in KINDS:
        x = values_of(c, vk)
        xs = None if x is None else x[perm]
        wj, wx = O.sort_sparse_indices(c.p, js, xs)
        assert np.array_equal(wj, c.j)
        j, xo, launch = dev_sort_rows(GCsr(c.p, js, xs), dt)
        assert launch == ("sort", c.G)
        same_csr((c.p, j, xo), (c.p, wj, wx), f"dtype {dt}")
        ej, ex = js.copy(), None if xs is None else xs.copy()
        G.sort_sparse_indices_inplace(c.p, ej, ex)
        assert last_row_launch() == ("sort", c.G)
        same_csr((c.p, ej, ex), (c.p, wj, wx), f"export dtype {dt}")


REVERSE = {MX_F64: G.reverse_columns_inplace_numeric, MX_LGL: G.reverse_columns_inplace_logical}


@pytest.mark.parametrize("c", HALF_CASES, ids=ids(HALF_CASES))
def test_reverse_columns(gpu, c):
    for dt, vk in KINDS:
        x = values_of(c, vk)
        wj, wx = c.j.copy(), None if x is None else x.copy()
        O.reverse_columns_inplace(c.p, wj, wx, c.K)
        j, xo, launch = dev_reverse_columns(GCsr(c.p, c.j, x), dt, c.K, c.nnz)
        assert launch == ("mxd_csr_reverse_columns", c.G)
        same_csr((c.p, j, xo), (c.p, wj, wx), f"dtype {dt}")
        ej, ex = c.j.copy(), None if x is None else x.copy()
        if dt == MX_NONE:
            G.reverse_columns_inplace_binary(c.p, ej, c.K)
        else:
            REVERSE[dt](c.p, ej, ex, c.K)
        assert last_row_launch() == ("mxd_csr_reverse_columns", c.G)
        same_csr((c.p, ej, ex), (c.p, wj, wx), f"export dtype {dt}")


# --------------------------------------------------------------------------------------- CSR x / (.) vector kernels
@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_spmv_svec(gpu, c):
    rng = np.random.default_rng([c.G, c.m, 9])
    yi = np.sort(rng.choice(c.K, size=c.K // 2, replace=False)).astype(np.int32) + 1
    yint = rng.integers(-4, 5, size=yi.size).astype(np.int32)
    yna = yint.copy()
    yna[rng.integers(0, yi.size, size=3)] = NA
    xi = c.vals["int"][0]
    A = GCsr(c.p, c.j, xi)
    kinds = ((0, yint.astype(np.float64), O.matmul_csr_svec_numeric, G.matmul_csr_svec_numeric),
             (1, yna, O.matmul_csr_svec_integer, G.matmul_csr_svec_integer),
             (2, yna, O.matmul_csr_svec_logical, G.matmul_csr_svec_logical),
             (3, None, O.matmul_csr_svec_binary, G.matmul_csr_svec_binary),
             (4, yint.astype(np.float32), O.matmul_csr_svec_float32, G.matmul_csr_svec_float32))
    for kind, yv, oracle, export in kinds:
        args = (c.p, c.j, xi, yi) if yv is None else (c.p, c.j, xi, yi, yv)
        want = oracle(*args)
        got, launch = dev_spmv_svec(A, yi, yv, kind, c.nnz)
        assert launch == ("mxd_spmv_csr_svec", c.G)
        same_values(got, want, f"kind {kind}")
        same_values(export(*args), want, f"export kind {kind}")
        assert last_row_launch() == ("mxd_spmv_csr_svec", c.G)
    # general data, numeric vector: the bound of the SpMV (f64 accumulation)
    xg = np.where(np.isfinite(c.vals["gen"][0]), c.vals["gen"][0], 1.5)
    yv = rng.normal(size=yi.size)
    vd = np.zeros(c.K)
    vd[yi - 1] = yv
    got, launch = dev_spmv_svec(GCsr(c.p, c.j, xg), yi, yv, 0, c.nnz)
    assert launch == ("mxd_spmv_csr_svec", c.G)
    check_sums(got, c, xg, vd, c.G, 2.0 ** -53, "svec")


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_by_dvec(gpu, c):
    rng = np.random.default_rng([c.G, c.m, 11])
    xg, xl = c.vals["gen"][0], c.vals["lgl"][0]
    A, Al = GCsr(c.p, c.j, xg), GCsr(c.p, c.j, xl)
    for length in (c.m, c.m * c.K, 7):                       # per row, the whole matrix, general recycling
        dv = rng.normal(size=length)
        dv[rng.integers(0, length, size=2)] = [0.0, np.inf]
        for op, flags, lhs in ((0, (True, False, False), True), (2, (False, False, True), True), (2, (False, False, True), False)):
            mul, pw, div = flags
            with np.errstate(all="ignore"):
                want = O.multiply_csr_by_dvec_no_NAs_numeric(c.p, c.j, xg, dv, c.K, mul, pw, div, False, False, lhs)
            got, launch = dev_by_dvec(A, c.K, dv, op, lhs, c.nnz)
            assert launch == ("mxd_csr_by_dvec", c.G)
            same_values(got, want, f"op {op} lhs {lhs} length {length}")
            same_values(G.multiply_csr_by_dvec_no_NAs_numeric(c.p, c.j, xg, dv, c.K, mul, pw, div, False, False, lhs), want)
            assert last_row_launch() == ("mxd_csr_by_dvec", c.G)
        dl = rng.choice(np.array([0, 1, NA], dtype=np.int32), size=length)
        want = O.logicaland_csr_by_dvec_internal(c.p, c.j, xl, dl, c.K)
        got, launch = dev_by_dvec(Al, c.K, dl, 5, True, c.nnz)
        assert launch == ("mxd_csr_by_dvec", c.G)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(G.logicaland_csr_by_dvec_internal(c.p, c.j, xl, dl, c.K), want)


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_by_svec(gpu, c):
    from test_gpu_svec_operands import check as check_svec, ref_mul
    rng = np.random.default_rng([c.G, c.m, 13])
    xg = c.vals["gen"][0]
    A = GCsr(c.p, c.j, xg)
    L = c.m
    vi = np.sort(rng.choice(L, size=max(1, L // 2), replace=False)).astype(np.int32) + 1
    vx = rng.normal(size=vi.size)
    if vi.size >= 4:
        vx[1], vx[2] = np.nan, np.inf
    for keep in (False, True):
        for v in (vx, None):
            want = ref_mul(c.p, c.j, xg, vi, v, L, c.K, keep)
            p, j, x, total, launches = dev_by_svec(A, c.K, vi, v, L, keep)
            assert launches == [("mxd_csr_by_svec_count", c.G), ("mxd_csr_by_svec_fill", c.G)]
            assert total == want[1].size
            check_svec((p, j, x), want, f"keep={keep} values={v is not None}")
            ex = (G.multiply_csr_by_svec_keep_NAs(c.p, c.j, xg, vi, v if v is not None else np.zeros(0), c.K, L) if keep
                  else G.multiply_csr_by_svec_no_NAs(c.p, c.j, xg, vi, v if v is not None else np.zeros(0), L))
            assert last_row_launch() == ("mxd_csr_by_svec_fill", c.G)
            check_svec(from_dict(ex), want, f"export keep={keep}")


# ------------------------------------------------------------------------------------------------------- hints only
def case_of(G, m=1003):
    return next(c for c in CASES if c.G == G and c.m == m)


def short_rows_case():
    """300 rows of at most 2 entries, and a partner of the same kind"""
    rng = np.random.default_rng(21)
    out = []
    for _ in range(2):
        lens = rng.integers(0, 3, size=300)
        p = np.zeros(301, dtype=np.int32)
        p[1:] = np.cumsum(lens)
        j = np.concatenate([np.sort(rng.choice(40, size=n, replace=False)) for n in lens]).astype(np.int32)
        out.append((p, j, rng.normal(size=j.size)))
    return out


HINT_MATRICES = ("long_rows_hint_4", "short_rows_hint_64", "unknown")


def hinted(which):
    """(A, partner, per-row hint or None): the matrix with 230-entry rows under a hint of 2 entries a row (4 lanes), rows
    of at most 2 entries under a hint of 64 a row (64 lanes), and the first matrix with the hint -1"""
    if which == "short_rows_hint_64":
        (p, j, x), (p2, j2, x2) = short_rows_case()
        return (p, j, x), (p2, j2, x2), 64
    c = case_of(16)
    return (c.p, c.j, c.vals["gen"][0]), (c.p2, c.j2, c.vals["gen"][1]), (2 if which == "long_rows_hint_4" else None)


@pytest.mark.parametrize("which", HINT_MATRICES)
def test_hints_only_steer_the_width(gpu, which):
    """mxd_spmv_csr_dvec, mxd_csr_merge_*, mxd_csr_gather_fill, mxd_csr_colrange_*, mxd_csr_colmap_* and mxd_csr_cbind
    read nnz / nnz_out / avg_row_len / nnz_total for the lane width alone (spmv.hip, merge.hip, gather.hip, colslice.hip,
    bind.hip): a wrong hint changes the reported G and nothing else.  -1 means 32 lanes where the header documents it
    (SpMV, merge, gather); the column slices and cbind hand it to pick_group, which gives 4."""
    (p, j, x), (p2, j2, x2), per_row = hinted(which)
    m, K = p.size - 1, int(max(j.max(), j2.max())) + 1
    nnz, nnz2 = j.size, j2.size
    h = (lambda rows, true: -1) if per_row is None else (lambda rows, true: per_row * rows)      # noqa: E731
    rng = np.random.default_rng(3)
    rt = np.concatenate([[0, m - 1], np.arange(m - 1, -1, -1), rng.integers(0, m, size=40)]).astype(np.int32)
    A, B = GCsr(p, j, x), GCsr(p2, j2, x2)
    # SpMV, on integer-valued data: another width sums in another order, which must not show
    with np.errstate(invalid="ignore"):
        Ai = GCsr(p, j, np.round(x))
    v = rng.integers(-4, 5, size=K).astype(np.float64)
    y0, _ = dev_spmv(Ai, v, MX_F64, nnz)
    y1, launch = dev_spmv(Ai, v, MX_F64, h(m, nnz))
    assert launch == ("spmv", R.spmv_group(m, h(m, nnz)))
    same_values(y1, y0, "spmv")
    # merge (6 ops would repeat the same launch shape: the union and the intersection)
    for op in (_lib.MX_OP_SUB, _lib.MX_OP_MUL):
        r0 = dev_merge(op, A, B, nnz, nnz2)
        r1 = dev_merge(op, A, B, h(m, nnz), h(m, nnz2))
        assert r1[4] == [("merge", R.merge_group(m, h(m, nnz), h(m, nnz2)))] * 2
        same_csr(r1[:3], r0[:3], f"merge op {op}")
    # gather
    nout = int(np.diff(p)[rt].sum())
    r0 = dev_gather(A, rt, MX_F64, nout)
    r1 = dev_gather(A, rt, MX_F64, h(rt.size, nout))
    assert r1[4] == ("gather", R.spmv_group(rt.size, h(rt.size, nout)))
    same_csr(r1[:3], r0[:3], "gather")
    # column slices: the hint is a mean row length
    avg, wrong = nnz / m, (-1.0 if per_row is None else float(per_row))
    lo, hi = int(j[0]), int(j[0]) + K // 2
    r0 = dev_colrange(A, rt, lo, hi, MX_F64, avg)
    r1 = dev_colrange(A, rt, lo, hi, MX_F64, wrong)
    assert r1[4] == [("mxd_csr_colrange_count", R.pick_group(wrong)), ("mxd_csr_colrange_fill", R.pick_group(wrong))]
    same_csr(r1[:3], r0[:3], "colrange")
    cols = rng.integers(0, K, size=K // 2).astype(np.int32)
    r0 = dev_colmap(A, rt, cols, MX_F64, avg)
    r1 = dev_colmap(A, rt, cols, MX_F64, wrong)
    assert r1[4] == [("mxd_csr_colmap_count", R.pick_group(wrong)), ("mxd_csr_colmap_fill", R.pick_group(wrong))]
    same_csr(r1[:3], r0[:3], "colmap")
    # cbind
    Y = GCsr(p2, (j2 + K).astype(np.int32), x2)
    r0 = dev_cbind(A, Y, MX_F64, nnz + nnz2)
    r1 = dev_cbind(A, Y, MX_F64, h(2 * m, nnz + nnz2))
    assert r1[3] == ("mxd_csr_cbind", R.half_group(m, h(2 * m, nnz + nnz2)))
    same_csr(r1[:3], r0[:3], "cbind")


# ------------------------------------------------------------------------------------------------------------- scan
SCAN_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 18 + 4097,
              2 ** 20 + 1, 2 ** 20 + 4096 * 3 + 5]


def scan_counts(n):
    """mostly 0..3, runs of zeros, a few values near 10^5"""
    rng = np.random.default_rng([n, 17])
    counts = rng.integers(0, 4, size=n).astype(np.int32)
    for s in rng.integers(0, max(n, 1), size=min(n, 12)):
        counts[s:s + int(rng.integers(1, 6000))] = 0
    if n:
        at = rng.integers(0, n, size=min(n, 9))
        counts[at] = 100000 - rng.integers(0, 50, size=at.size).astype(np.int32)
        counts[-1] = 3                                      # the last element counts too
    return counts


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan(gpu, n):
    counts = scan_counts(n)
    want = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    assert want[-1] < 2 ** 31
    out, total = dev_scan(counts)
    assert total == int(want[-1])
    np.testing.assert_array_equal(out, want.astype(np.int32))


def test_count_total_beyond_int32_is_refused(gpu):
    """40 000 copies of one 70 000-entry row: only indptr is read; the 64-bit total comes back and the call fails"""
    lib = _lib.load()
    r = 40000
    gp, grows = GuardedVec(np.int32, data=np.array([0, 70000], dtype=np.int32)), GuardedVec(np.int32, data=np.zeros(r, np.int32))
    gout, gws = GuardedVec(np.int32, n=r + 1), GuardedVec(np.uint8, n=lib.mxd_gather_workspace_bytes(r))
    total = C.c_int64(-1)
    rc = lib.mxd_csr_gather_count(C.c_int(r), gp.ptr, grows.ptr, gout.ptr, gws.ptr, C.byref(total), None)
    assert rc != 0
    assert "exceeds R's int32 index range" in lib.mx_last_error().decode()
    assert total.value == 2_800_000_000
    _lib.check(lib.mx_stream_sync(None))
    gp.assert_untouched()
    grows.assert_untouched()
    gout.result()                                           # guards intact; the (wrapped) offsets were all written
    gws._download()


# -------------------------------------------------------------------------------------------------------- grid caps
@pytest.mark.parametrize("n", [600_000, 1_300_000])
@pytest.mark.parametrize("rev", [False, True])
def test_check_is_seq_beyond_one_grid(gpu, n, rev):
    """is_seq_kernel runs 2048 x 256 = 524 288 lanes: elements from 524 289 on belong to the later trips of its loop"""
    fn, oracle = (G.check_is_rev_seq, O.check_is_rev_seq) if rev else (G.check_is_seq, O.check_is_seq)
    clean = (np.arange(n, 0, -1) if rev else np.arange(7, n + 7)).astype(np.int32)
    assert fn(clean) is True and oracle(clean)
    spots = [524288, 524288 + 40_000] + ([2 * 524288 + 100_000] if n > 2 * 524288 + 100_000 else [])
    for at in spots:                                        # the pair (at - 1, at) alone breaks the sequence
        bad = clean.copy()
        bad[at:] += 1 if not rev else -1
        assert not oracle(bad)
        assert fn(bad) is False, f"violation at {at} of {n} not seen"


def test_rows_sorted_beyond_one_grid(gpu):
    """rows_sorted_kernel runs 4096 x 256 = 1 048 576 lanes"""
    m, per = 2100, 512
    p = (np.arange(m + 1) * per).astype(np.int32)
    j = np.tile(np.arange(per, dtype=np.int32) * 2, m)
    assert j.size > 1048576
    assert G.check_indices_are_sorted(p, j) is True and O.check_indices_are_sorted(p, j)
    bad = j.copy()
    k = 1048576 + 11_000
    assert k % per not in (0, per - 1)
    bad[k], bad[k + 1] = bad[k + 1], bad[k]
    assert not O.check_indices_are_sorted(p, bad)
    assert G.check_indices_are_sorted(p, bad) is False
    # the only descent crosses a row boundary that follows empty rows: sorted
    lens = np.full(m, per)
    lens[[1000, 1001, 1002]] = 0
    p2 = np.zeros(m + 1, dtype=np.int32)
    p2[1:] = np.cumsum(lens)
    j2 = np.concatenate([np.arange(n, dtype=np.int32) + (5 if r < 1000 else 0) for r, n in enumerate(lens)])
    assert O.check_indices_are_sorted(p2, j2)
    assert G.check_indices_are_sorted(p2, j2) is True


def test_values_elemwise_beyond_one_grid(gpu):
    """values_elemwise_kernel runs 4096 x 256 lanes; reached through the identical-structure path of the exports"""
    rng = np.random.default_rng(23)
    n, m = 1048576 + 70_001, 1000
    p = np.linspace(0, n, m + 1).astype(np.int32)
    j = np.concatenate([np.arange(e - s, dtype=np.int32) for s, e in zip(p[:-1], p[1:])])
    x1, x2 = rng.normal(size=n), rng.normal(size=n)
    x1[-5:] = [0.0, -0.0, np.inf, np.nan, 1.0]
    x2[-5:] = [-0.0, -0.0, -np.inf, 1.0, np.nan]
    with np.errstate(all="ignore"):
        got = G.add_csr_elemwise(p, p, j, j, x1, x2, True)
        assert got["indptr"] is p and got["indices"] is j
        same_values(got["values"], x1 + (-x2))
        same_values(G.multiply_csr_elemwise(p, p, j, j, x1, x2)["values"], x1 * x2)
    l1 = rng.choice(np.array([0, 1, NA], dtype=np.int32), size=n)
    l2 = rng.choice(np.array([0, 1, NA], dtype=np.int32), size=n)
    from test_row_group_cases import r_logical
    np.testing.assert_array_equal(G.logicalor_csr_elemwise(p, p, j, j, l1, l2, False)["values"], r_logical("or", l1, l2))
    np.testing.assert_array_equal(G.logicaland_csr_elemwise(p, p, j, j, l1, l2)["values"], r_logical("and", l1, l2))
