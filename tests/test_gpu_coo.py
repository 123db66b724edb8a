"""COO (TsparseMatrix) on the device: COO -> CSR / CSC (mxd_coo_to_csr), CSR / CSC -> COO (mxd_csr_to_coo),
CSR (.) COO (mxd_csr_by_coo_*), COO (op) vector (mxd_coo_by_dvec) and the operators built on them.

Expected results come from a numpy restatement that follows the reference and Matrix's triplet coercion:
np.lexsort((j, i)) (stable) orders the triplets by row, then column, in input order; repeated (i, j) pairs are
merged in that order (f64 by a left-to-right sum, the same order np.add.at adds in; R logicals by R's `|`;
pattern once).  Values are compared bit for bit, so NA_real_ and other NaN payloads stay distinct.
"""
import warnings

import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G
from conftest import rand_csr

pytestmark = pytest.mark.gpu

NA_LGL = np.int32(-2147483648)
NA_REAL = mx.NA_REAL
OTHER_NAN = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0]


def _r_or(a, b):
    if a == NA_LGL:
        return NA_LGL if b == NA_LGL else (1 if b else NA_LGL)
    if b == NA_LGL:
        return 1 if a else NA_LGL
    return int(a != 0 or b != 0)


def _r_and(a, b):
    if a == NA_LGL:
        return NA_LGL if b == NA_LGL else (NA_LGL if b else 0)
    if b == NA_LGL:
        return NA_LGL if a else 0
    return int(a != 0 and b != 0)


def ref_coo_to_csr(i, j, x, m, n):
    i, j = np.asarray(i, np.int32), np.asarray(j, np.int32)
    order = np.lexsort((j, i))
    ri, cj = i[order], j[order]
    vals = None if x is None else np.asarray(x)[order]
    head = np.ones(ri.size, dtype=bool)
    head[1:] = (ri[1:] != ri[:-1]) | (cj[1:] != cj[:-1])
    starts = np.flatnonzero(head)
    if vals is not None and not head.all():
        if vals.dtype == np.float64:
            # np.add.at adds in index order: the input-order sum, bit for bit
            grp = np.cumsum(head) - 1
            merged = np.zeros(starts.size)
            merged[:] = vals[starts]
            rest = np.flatnonzero(~head)
            np.add.at(merged, grp[rest], vals[rest])
        else:
            ends = np.append(starts[1:], ri.size)
            merged = vals[starts].copy()
            for g in np.flatnonzero(ends - starts > 1):
                acc = vals[starts[g]]
                for e in range(starts[g] + 1, ends[g]):
                    acc = _r_or(acc, vals[e])
                merged[g] = acc
        vals = merged
    elif vals is not None:
        vals = vals[starts]
    ri, cj = ri[starts], cj[starts]
    indptr = np.zeros(m + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(ri, minlength=m))
    return indptr, cj.astype(np.int32), vals


def assert_bits(got, want):
    if want is None:
        assert got is None
        return
    assert got.dtype == want.dtype and got.shape == want.shape
    if want.dtype == np.float64:
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    else:
        assert np.array_equal(got, want)


def check_coo_to_csr(i, j, x, m, n):
    got = G.coo_to_csr(i, j, x, m, n)
    p, jj, xx = ref_coo_to_csr(i, j, x, m, n)
    assert np.array_equal(got["indptr"], p)
    assert np.array_equal(got["indices"], jj)
    assert_bits(got["values"], xx)
    return got


def rand_coo(m, n, nnz, seed, dup_share=0.0, kind="d"):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, m, nnz).astype(np.int32)
    j = rng.integers(0, n, nnz).astype(np.int32)
    ndup = int(nnz * dup_share)
    if ndup:
        src = rng.integers(0, nnz - ndup, ndup)
        i[nnz - ndup:], j[nnz - ndup:] = i[src], j[src]
        perm = rng.permutation(nnz)
        i, j = i[perm], j[perm]
    if kind == "d":
        x = np.round(rng.normal(size=nnz), 3)
    elif kind == "l":
        x = rng.choice(np.array([0, 1, NA_LGL], dtype=np.int32), size=nnz, p=[0.3, 0.5, 0.2])
    else:
        x = None
    return i, j, x


# ----------------------------------------------------------------------------- COO -> CSR
@pytest.mark.parametrize("kind", ["d", "l", "n"])
def test_shuffled_with_duplicates(gpu, kind):
    i, j, x = rand_coo(300, 200, 20000, 1, dup_share=0.3, kind=kind)
    got = check_coo_to_csr(i, j, x, 300, 200)
    assert got["indices"].size < i.size


def test_all_entries_identical(gpu):
    n = 9000
    i, j = np.full(n, 3, np.int32), np.full(n, 5, np.int32)
    x = np.random.default_rng(2).normal(size=n)
    got = check_coo_to_csr(i, j, x, 7, 8)
    assert got["indices"].tolist() == [5]
    lg = check_coo_to_csr(i, j, np.where(np.arange(n) == 17, NA_LGL, 0).astype(np.int32), 7, 8)
    assert lg["values"].tolist() == [NA_LGL]
    check_coo_to_csr(i, j, None, 7, 8)


def test_explicit_zeros_are_kept(gpu):
    i = np.array([0, 0, 1], np.int32)
    j = np.array([1, 1, 0], np.int32)
    got = check_coo_to_csr(i, j, np.array([2.5, -2.5, 0.0]), 2, 2)
    assert got["values"].tolist() == [0.0, 0.0] and got["indices"].tolist() == [1, 0]


@pytest.mark.parametrize("m, n", [(5, 4), (0, 4), (5, 0), (0, 0)])
def test_empty(gpu, m, n):
    e = np.zeros(0, np.int32)
    check_coo_to_csr(e, e, np.zeros(0), m, n)
    check_coo_to_csr(e, e, None, m, n)


def test_hot_row_and_hot_column(gpu):
    rng = np.random.default_rng(3)
    m, n = 5000, 4000
    i = np.concatenate([np.full(n, 17), np.arange(m), rng.integers(0, m, 30000)]).astype(np.int32)
    j = np.concatenate([np.arange(n), np.full(m, 9), rng.integers(0, n, 30000)]).astype(np.int32)
    perm = rng.permutation(i.size)
    check_coo_to_csr(i[perm], j[perm], rng.normal(size=i.size), m, n)


@pytest.mark.parametrize("n", [200, 300, 70000, (1 << 24) + 5])
def test_digit_pass_counts(gpu, n):
    # n > 256 / 2^16 / 2^24 makes the column sort run two / three / four digit passes; m does the same for rows
    m = n
    i, j, x = rand_coo(m, n, 30000, 4, dup_share=0.1)
    check_coo_to_csr(i, j, x, m, n)
    check_coo_to_csr(j, i, x, n, m)


def test_many_tiles(gpu):
    i, j, x = rand_coo(2000, 3000, 200_000, 5, dup_share=0.1)
    check_coo_to_csr(i, j, x, 2000, 3000)


def test_nan_payloads_are_copied(gpu):
    i = np.array([2, 0, 1, 0], np.int32)
    j = np.array([1, 3, 0, 0], np.int32)
    x = np.array([NA_REAL, OTHER_NAN, -0.0, 1.0])
    check_coo_to_csr(i, j, x, 3, 4)


def test_logical_na_under_or(gpu):
    i = np.array([0, 0, 0, 0, 1, 1, 2, 2], np.int32)
    j = np.array([0, 0, 1, 1, 0, 0, 2, 2], np.int32)
    x = np.array([NA_LGL, 1, NA_LGL, 0, 0, 0, NA_LGL, NA_LGL], np.int32)
    got = check_coo_to_csr(i, j, x, 3, 3)
    assert got["values"].tolist() == [1, NA_LGL, 0, NA_LGL]


@pytest.mark.parametrize("bad", [(0, 4), (3, 0), (-1, 0), (0, -1)])
def test_index_out_of_range_fails(gpu, bad):
    i = np.array([0, 1, 2, bad[0]], np.int32)
    j = np.array([0, 1, 2, bad[1]], np.int32)
    with pytest.raises(_lib.MxError, match="outside"):
        G.coo_to_csr(i, j, np.ones(4), 3, 4)
    # the process and the device are intact
    check_coo_to_csr(i[:3], j[:3], np.ones(3), 3, 4)


def test_as_csr_value_types_convert_after_merge(gpu):
    i = np.array([0, 0, 1, 1, 1], np.int32)
    j = np.array([1, 1, 0, 0, 2], np.int32)
    n = mx.as_csr_matrix(mx.ngTMatrix(i, j, None, (2, 3)))
    assert type(n) is mx.dgRMatrix and n.x.tolist() == [1.0, 1.0, 1.0]
    lg = mx.lgTMatrix(i, j, np.array([NA_LGL, 0, NA_LGL, 1, 0], np.int32), (2, 3))
    d = mx.as_csr_matrix(lg)
    assert type(d) is mx.dgRMatrix
    assert_bits(d.x, np.array([NA_REAL, 1.0, 0.0]))
    dg = mx.dgTMatrix(i, j, np.array([2.0, -2.0, 0.5, np.nan, 0.0]), (2, 3))
    lo = mx.as_csr_matrix(dg, logical=True)
    assert type(lo) is mx.lgRMatrix and lo.x.tolist() == [0, NA_LGL, 0]
    b = mx.as_csr_matrix(dg, binary=True)
    assert type(b) is mx.ngRMatrix and b.j.tolist() == [1, 0, 2]


def test_round_trips(gpu):
    p, j, x = rand_csr(60, 45, 0.2, 6)
    X = mx.dgRMatrix(p, j, x, (60, 45))
    T = mx.as_coo_matrix(X)
    assert type(T) is mx.dgTMatrix and T.Dim == X.Dim
    assert np.array_equal(T.i, np.repeat(np.arange(60), np.diff(p))) and T.j is X.j
    back = mx.as_csr_matrix(T)
    assert np.array_equal(back.p, p) and np.array_equal(back.j, j) and np.array_equal(back.x.view(np.uint64),
                                                                                        x.view(np.uint64))
    i2, j2, x2 = rand_coo(40, 70, 3000, 7, dup_share=0.3)
    T2 = mx.dgTMatrix(i2, j2, x2, (40, 70))
    C = mx.as_csc_matrix(T2)
    R = mx.as_csr_matrix(T2.t())
    assert type(C) is mx.dgCMatrix and C.Dim == (40, 70)
    assert np.array_equal(C.p, R.p) and np.array_equal(C.i, R.j)
    assert np.array_equal(C.x.view(np.uint64), R.x.view(np.uint64))
    # CSC -> COO is column-major, as Matrix gives it
    TC = mx.as_coo_matrix(C)
    assert np.array_equal(TC.j, np.repeat(np.arange(70), np.diff(C.p))) and TC.i is C.i
    np.testing.assert_allclose(TC.toarray(), T2.toarray())


def test_as_coo_flags(gpu):
    p, j, x = rand_csr(10, 8, 0.4, 8, dtype="l")
    L = mx.lgRMatrix(p, j, x, (10, 8))
    d = mx.as_coo_matrix(L)
    assert type(d) is mx.dgTMatrix
    assert_bits(d.x, np.where(x == NA_LGL, NA_REAL, x.astype(np.float64)))
    assert mx.as_coo_matrix(d, logical=True).x.tolist() == [NA_LGL if v == NA_LGL else int(v != 0) for v in x]
    assert type(mx.as_coo_matrix(L, binary=True)) is mx.ngTMatrix
    assert mx.as_coo_matrix(d) is d


# ----------------------------------------------------------------------------- CSR (.) COO
def ref_csr_by_coo(X, i, j, y, logical):
    rows, cols, vals = [], [], []
    m, n = X.Dim
    for k in range(i.size):
        yk = y[k]
        if (yk == 0) if logical else not (np.isnan(yk) or yk != 0):
            continue
        if not (0 <= i[k] < m and 0 <= j[k] < n):
            continue
        s, e = X.p[i[k]], X.p[i[k] + 1]
        hit = np.flatnonzero(X.j[s:e] == j[k])
        if not hit.size:
            continue
        xv = X.x[s + hit[0]]
        if (xv == 0) if logical else not (np.isnan(xv) or xv != 0):
            continue
        rows.append(i[k])
        cols.append(j[k])
        vals.append(_r_and(xv, yk) if logical else xv * yk)
    return (np.array(rows, np.int32), np.array(cols, np.int32),
            np.array(vals, np.int32 if logical else np.float64))


def test_csr_times_coo_values(gpu):
    X = mx.dgRMatrix(np.array([0, 3, 4, 6], np.int32), np.array([0, 2, 3, 1, 0, 3], np.int32),
                     np.array([2.0, 0.0, np.nan, 5.0, -1.0, 4.0]), (3, 4))
    i = np.array([0, 0, 0, 1, 2, 2, 0, 1, 5, 2, 2], np.int32)
    j = np.array([0, 2, 3, 1, 3, 0, 0, 0, 0, 9, 3], np.int32)
    y = np.array([3.0, 7.0, 1.0, np.nan, 0.0, 2.0, 3.0, 1.0, 1.0, 1.0, NA_REAL])
    res = G.multiply_csr_by_coo_elemwise(X.p, X.j, X.x, i, j, y, 3, 4)
    r, c, v = ref_csr_by_coo(X, i, j, y, False)
    assert np.array_equal(res["row"], r) and np.array_equal(res["col"], c)
    assert_bits(res["val"], v)
    assert res["row"].tolist() == [0, 0, 1, 2, 0, 2]          # input order, the duplicate (0, 0) twice


def test_csr_and_coo_logical(gpu):
    p, j, x = rand_csr(30, 20, 0.3, 9, dtype="l")
    X = mx.lgRMatrix(p, j, x, (30, 20))
    i2, j2, y = rand_coo(35, 25, 800, 10, dup_share=0.2, kind="l")
    res = G.logicaland_csr_by_coo_elemwise(X.p, X.j, X.x, i2, j2, y, 30, 20)
    r, c, v = ref_csr_by_coo(X, i2, j2, y, True)
    assert np.array_equal(res["row"], r) and np.array_equal(res["col"], c) and np.array_equal(res["val"], v)


def test_csr_times_coo_bigger_dims_warns(gpu):
    p, j, x = rand_csr(20, 15, 0.4, 11)
    X = mx.dgRMatrix(p, j, x, (20, 15))
    i2, j2, y = rand_coo(25, 18, 500, 12, dup_share=0.1)
    T = mx.dgTMatrix(i2, j2, y, (25, 18))
    with pytest.warns(UserWarning, match="Matrices to multiply have different dimensions."):
        out = X * T
    assert type(out) is mx.dgTMatrix and out.Dim == (25, 18) and out.Dimnames == [None, None]
    r, c, v = ref_csr_by_coo(X, i2, j2, y, False)
    assert np.array_equal(out.i, r) and np.array_equal(out.j, c)
    assert_bits(out.x, v)


# ----------------------------------------------------------------------------- operators, test-operators.R:217-278
def _pair(seed):
    p1, j1, x1 = rand_csr(25, 18, 0.3, seed)
    p2, j2, x2 = rand_csr(25, 18, 0.3, seed + 1)
    return mx.dgRMatrix(p1, j1, x1, (25, 18)), mx.dgRMatrix(p2, j2, x2, (25, 18))


def _dense_or(a, b):
    return ((a != 0) | (b != 0)).astype(np.float64)


def test_operations_csr_coo(gpu):
    csr1, csr2 = _pair(20)
    emat = mx.dgRMatrix(np.zeros(26, np.int32), np.zeros(0, np.int32), np.zeros(0), (25, 18))
    mat1, mat2, eden = csr1.toarray(), csr2.toarray(), np.zeros((25, 18))
    coo1 = mx.as_coo_matrix(csr1)
    cases = [
        (lambda: coo1 + csr2, mat1 + mat2, mx.dgRMatrix), (lambda: coo1 + emat, mat1 + eden, mx.dgRMatrix),
        (lambda: csr2 + coo1, mat2 + mat1, mx.dgRMatrix), (lambda: emat + coo1, eden + mat1, mx.dgRMatrix),
        (lambda: coo1 - csr2, mat1 - mat2, mx.dgRMatrix), (lambda: coo1 - emat, mat1 - eden, mx.dgRMatrix),
        (lambda: csr2 - coo1, mat2 - mat1, mx.dgRMatrix), (lambda: emat - coo1, eden - mat1, mx.dgRMatrix),
        (lambda: coo1 * csr2, mat1 * mat2, mx.dgTMatrix), (lambda: coo1 * emat, mat1 * eden, mx.dgTMatrix),
        (lambda: csr2 * coo1, mat2 * mat1, mx.dgTMatrix), (lambda: emat * coo1, eden * mat1, mx.dgTMatrix),
        (lambda: coo1 | csr2, _dense_or(mat1, mat2), mx.lgRMatrix),
        (lambda: coo1 | emat, _dense_or(mat1, eden), mx.lgRMatrix),
        (lambda: csr2 | coo1, _dense_or(mat2, mat1), mx.lgRMatrix),
        (lambda: emat | coo1, _dense_or(eden, mat1), mx.lgRMatrix),
        (lambda: coo1 & csr2, ((mat1 != 0) & (mat2 != 0)).astype(float), mx.lgTMatrix),
        (lambda: coo1 & emat, np.zeros((25, 18)), mx.lgTMatrix),
        (lambda: csr2 & coo1, ((mat2 != 0) & (mat1 != 0)).astype(float), mx.lgTMatrix),
        (lambda: emat & coo1, np.zeros((25, 18)), mx.lgTMatrix),
        (lambda: coo1 ** 2, mat1 ** 2, mx.dgTMatrix),
    ]
    for k, (f, want, cls) in enumerate(cases):
        got = f()
        assert type(got) is cls, k
        np.testing.assert_array_equal(got.toarray(), want, err_msg=str(k))


def test_operations_csc_coo(gpu):
    csr1, csr2 = _pair(30)
    mat1, mat2 = csr1.toarray(), csr2.toarray()
    csc2 = mx.as_csc_matrix(csr2)
    coo1 = mx.as_coo_matrix(csr1)
    for f, want, cls in [(lambda: csc2 + coo1, mat2 + mat1, mx.dgCMatrix),
                         (lambda: coo1 + csc2, mat1 + mat2, mx.dgCMatrix),
                         (lambda: csc2 - coo1, mat2 - mat1, mx.dgCMatrix),
                         (lambda: coo1 - csc2, mat1 - mat2, mx.dgCMatrix),
                         (lambda: csc2 * coo1, mat2 * mat1, mx.dgTMatrix),
                         (lambda: coo1 * csc2, mat1 * mat2, mx.dgTMatrix),
                         (lambda: csc2 & coo1, ((mat2 != 0) & (mat1 != 0)).astype(float), mx.lgTMatrix)]:
        got = f()
        assert type(got) is cls
        dense = mx.as_csr_matrix(got).toarray() if cls is mx.dgCMatrix else got.toarray()
        np.testing.assert_array_equal(dense, want)


# ----------------------------------------------------------------------------- COO (op) vector
def _storage_order_values(X, T_out):
    """the COO result's values in the CSR's storage order (as_coo of a CSR keeps that order)"""
    return T_out.x


@pytest.mark.parametrize("vlen", ["nrow", "full", "divides", "other"])
@pytest.mark.parametrize("op", ["*", "/", "^", "%%", "%/%", "&"])
def test_coo_op_vector_matches_csr(gpu, vlen, op):
    m, n = 12, 7
    p, j, x = rand_csr(m, n, 0.5, 40)
    x = np.abs(x) + 0.25
    X = mx.dgRMatrix(p, j, x, (m, n))
    L = {"nrow": m, "full": m * n, "divides": 4, "other": 5}[vlen]
    v = np.random.default_rng(41).uniform(0.5, 3.0, L).round(2)
    T = mx.as_coo_matrix(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if op == "&":
            vl = (np.arange(L) % 3 != 0)
            want, got = X & vl, T & vl
            assert type(got) is mx.lgTMatrix
            assert np.array_equal(got.x, want.x)
            return
        fn = {"*": lambda a, b: a * b, "/": lambda a, b: a / b, "^": lambda a, b: a ** b,
              "%%": lambda a, b: a % b, "%/%": lambda a, b: a // b}[op]
        want, got = fn(X, v), fn(T, v)
        assert type(got) is mx.dgTMatrix and got.i is T.i and got.j is T.j
        assert np.array_equal(got.x.view(np.uint64), want.x.view(np.uint64))
        if op == "*":
            got_r = v * T
            assert np.array_equal(got_r.x.view(np.uint64), (v * X).x.view(np.uint64))


def test_coo_vector_routes_not_accelerated(gpu):
    T = mx.as_coo_matrix(mx.dgRMatrix(*rand_csr(6, 5, 0.5, 42), (6, 5)))
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        T * np.array([1.0, np.nan, 2.0])
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        np.array([1.0, 2.0, 3.0]) / T


def test_coo_dvec_export_matches_csr_export(gpu):
    p, j, x = rand_csr(50, 30, 0.3, 43)
    i = G.csr_to_coo(p)
    v = np.random.default_rng(44).uniform(-2, 2, 37)
    for flags in [(1, 0, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0)]:
        for lhs in (True, False):
            a = G.multiply_coo_by_dense_ignore_NAs_numeric(i, j, x, v, 50, 30, *flags, lhs)
            b = G.multiply_csr_by_dvec_no_NAs_numeric(p, j, x, v, 30, *flags, lhs)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ----------------------------------------------------------------------------- device API
def test_device_api_matches_exports(gpu):
    import torch
    from matrixextra_amd import device as D
    i, j, x = rand_coo(400, 300, 20000, 50, dup_share=0.3)
    A = D.coo_to_csr(torch.from_numpy(i).cuda(), torch.from_numpy(j).cuda(), torch.from_numpy(x).cuda(), 400, 300)
    want = G.coo_to_csr(i, j, x, 400, 300)
    hp, hj, hx = A.to_host()
    assert A.m == 400 and A.K == 300 and A.nnz == want["indices"].size
    assert np.array_equal(hp, want["indptr"]) and np.array_equal(hj, want["indices"])
    assert np.array_equal(hx.view(np.uint64), want["values"].view(np.uint64))
    rows, cols, vals = D.csr_to_coo(A)
    T = mx.as_coo_matrix(mx.dgRMatrix(hp, hj, hx, (400, 300)))
    assert np.array_equal(rows.cpu().numpy(), T.i) and np.array_equal(rows.cpu().numpy(), G.csr_to_coo(hp))
    assert cols is A.indices and vals is A.values
