"""remove_sparse_zeros, filterSparse, check_sparse_matrix and their exports on the device (compact.hip through
mxd_compact_count / _fill and mxd_validate_indices).

Expected results come from a numpy restatement of the reference's loops (src/misc.cpp:553-1116, R/utils.R:582-681),
written here from DESIGN.md §4.9's keep-rule table:

    routine                 removed without na.rm     removed with na.rm
    CSR / CSC numeric       x == 0                    x == 0 or NaN
    CSR / CSC logical       FALSE                     only NA (FALSE kept)
    COO numeric / logical   x == 0 / FALSE            also NaN / NA
    svec numeric            x == 0                    only x == 0 (NaN kept)
    svec integer / logical  0 / FALSE                 also NA

Kept entries stay in input order; a CSR's new indptr is the kept count before each old row start.  Values are
compared bit for bit (view as uint64), so NA_real_ and other NaN payloads stay distinct.
"""
import numpy as np
import pytest
import torch

import matrixextra_amd as mx
from matrixextra_amd import exports as G, synth
from conftest import rand_csr

pytestmark = pytest.mark.gpu

NA = np.int32(-2147483648)
NA_REAL = mx.NA_REAL
OTHER_NAN = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0]


# ---------------------------------------------------------------------------------------------- restatement
def ref_keep(layout, kind, x, na_rm):
    x = np.asarray(x)
    if kind == "d":
        nz, nn = x != 0, ~np.isnan(x)
        if not na_rm or layout == "svec":
            return nz
        return nz & nn
    nz, nn = x != 0, x != NA
    if not na_rm:
        return nz
    if layout == "csr" and kind == "l":
        return nn
    return nz & nn


def ref_indptr(p, keep):
    c = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    return c[np.asarray(p, np.int64)].astype(np.int32)


def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype == np.float64:
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    else:
        np.testing.assert_array_equal(a, b)


def values_of(kind, n, rng, zero_frac=0.3):
    if kind == "d":
        x = np.round(rng.normal(size=n), 2)
        x[x == 0] = 0.25
        r = rng.random(n)
        x[r < zero_frac] = 0.0
        x[(r >= zero_frac) & (r < zero_frac + 0.05)] = -0.0
        x[(r >= zero_frac + 0.05) & (r < zero_frac + 0.1)] = NA_REAL
        x[(r >= zero_frac + 0.1) & (r < zero_frac + 0.15)] = OTHER_NAN
        return x
    if kind == "l":
        return rng.choice(np.array([0, 1, NA], np.int32), size=n, p=[zero_frac, 0.85 - zero_frac, 0.15])
    return rng.choice(np.array([0, 7, -3, NA], np.int32), size=n, p=[zero_frac, 0.45 - zero_frac / 2,
                                                                     0.4 - zero_frac / 2, 0.15])


def csr_cases():
    rng = np.random.default_rng(11)
    p, j, _ = rand_csr(40, 30, 0.3, 3, sorted_cols=False, empty_rows=(0, 7, 39))
    yield "unsorted+empty", p, j, rng
    yield "nrow0", np.zeros(1, np.int32), np.zeros(0, np.int32), rng
    yield "nnz0", np.zeros(6, np.int32), np.zeros(0, np.int32), rng
    # rows across many tiles: ~20 000 entries, rows of varied length
    lens = rng.integers(0, 60, size=700)
    pp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    yield "multi-tile", pp, rng.integers(0, 500, size=pp[-1]).astype(np.int32), rng


# ---------------------------------------------------------------------------------------------- exports
@pytest.mark.parametrize("kind", ["d", "l"])
@pytest.mark.parametrize("na_rm", [False, True])
def test_remove_zero_valued_csr(gpu, kind, na_rm):
    fn = G.remove_zero_valued_csr_numeric if kind == "d" else G.remove_zero_valued_csr_logical
    for name, p, j, rng in csr_cases():
        x = values_of(kind, j.size, rng)
        keep = ref_keep("csr", kind, x, na_rm)
        out = fn(p, j, x, na_rm)
        if keep.all():                                       # the inputs themselves (misc.cpp:586-590)
            assert out["indptr"] is p and out["indices"] is j and out["values"] is x, name
            continue
        np.testing.assert_array_equal(out["indptr"], ref_indptr(p, keep), err_msg=name)
        np.testing.assert_array_equal(out["indices"], j[keep], err_msg=name)
        same_values(out["values"], x[keep])


@pytest.mark.parametrize("kind", ["d", "l"])
@pytest.mark.parametrize("na_rm", [False, True])
def test_remove_zero_valued_coo(gpu, kind, na_rm):
    fn = G.remove_zero_valued_coo_numeric if kind == "d" else G.remove_zero_valued_coo_logical
    rng = np.random.default_rng(5)
    for n in (0, 1, 37, 4096, 4097, 50_000):
        i = rng.integers(0, 300, n).astype(np.int32)
        j = rng.integers(0, 200, n).astype(np.int32)
        x = values_of(kind, n, rng)
        keep = ref_keep("coo", kind, x, na_rm)
        out = fn(i, j, x, na_rm)
        if keep.all():
            assert out["ii"] is i and out["jj"] is j and out["xx"] is x
            continue
        np.testing.assert_array_equal(out["ii"], i[keep])
        np.testing.assert_array_equal(out["jj"], j[keep])
        same_values(out["xx"], x[keep])


@pytest.mark.parametrize("kind", ["d", "i", "l"])
@pytest.mark.parametrize("na_rm", [False, True])
def test_remove_zero_valued_svec(gpu, kind, na_rm):
    fn = {"d": G.remove_zero_valued_svec_numeric, "i": G.remove_zero_valued_svec_integer,
          "l": G.remove_zero_valued_svec_logical}[kind]
    rng = np.random.default_rng(9)
    for n in (0, 5, 9000):
        ii = np.sort(rng.choice(10 * n + 10, n, replace=False)).astype(np.int32) + 1
        x = values_of(kind, n, rng)
        keep = ref_keep("svec", kind, x, na_rm)
        out = fn(ii, x, na_rm)
        if keep.all():
            assert out["ii"] is ii and out["xx"] is x
            continue
        np.testing.assert_array_equal(out["ii"], ii[keep])
        same_values(out["xx"], x[keep])
    # the svec numeric quirk: na.rm keeps NaN (misc.cpp:882-886)
    out = G.remove_zero_valued_svec_numeric(np.array([1, 2, 3], np.int32), np.array([NA_REAL, 0.0, 2.0]), True)
    same_values(out["xx"], np.array([NA_REAL, 2.0]))


def test_logical_csr_na_rm_quirk(gpu):
    p, j = np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32)
    out = G.remove_zero_valued_csr_logical(p, j, np.array([0, NA, 1], np.int32), True)   # FALSE kept, NA removed
    np.testing.assert_array_equal(out["indptr"], [0, 2])
    np.testing.assert_array_equal(out["values"], [0, 1])
    x = np.array([0, 1, 1], np.int32)          # FALSE and no NA: nothing removed, equal values (aliased here)
    same_values(G.remove_zero_valued_csr_logical(p, j, x, True)["values"], x)


def test_everything_removed_and_rows_emptied(gpu):
    p = np.array([0, 2, 2, 5, 6], np.int32)
    j = np.array([1, 3, 0, 2, 3, 1], np.int32)
    out = G.remove_zero_valued_csr_numeric(p, j, np.zeros(6), False)
    np.testing.assert_array_equal(out["indptr"], np.zeros(5, np.int32))
    assert out["indices"].size == 0 and out["values"].size == 0 and out["values"].dtype == np.float64
    x = np.array([0.0, -0.0, 1.0, 2.0, 3.0, 0.0])               # rows 0 and 3 lose every entry
    out = G.remove_zero_valued_csr_numeric(p, j, x, False)
    np.testing.assert_array_equal(out["indptr"], [0, 0, 0, 3, 3])
    np.testing.assert_array_equal(out["indices"], [0, 2, 3])


def test_skewed_row_crossing_many_tiles(gpu):
    rng = np.random.default_rng(2)
    lens = np.array([0, 0, 3, 1_200_000, 0, 0, 5, 0], np.int64)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = rng.integers(0, 100_000, p[-1]).astype(np.int32)
    x = values_of("d", p[-1], rng)
    for na_rm in (False, True):
        keep = ref_keep("csr", "d", x, na_rm)
        out = G.remove_zero_valued_csr_numeric(p, j, x, na_rm)
        np.testing.assert_array_equal(out["indptr"], ref_indptr(p, keep))
        np.testing.assert_array_equal(out["indices"], j[keep])
        same_values(out["values"], x[keep])


def test_rebuild_indptr_after_filter(gpu):
    for name, p, j, rng in csr_cases():
        f = rng.choice(np.array([0, 1, NA], np.int32), size=j.size)
        np.testing.assert_array_equal(G.rebuild_indptr_after_filter(p, f), ref_indptr(p, f != 0), err_msg=name)
    assert G.rebuild_indptr_after_filter(np.zeros(0, np.int32), np.zeros(0, np.int32)).size == 0


# ---------------------------------------------------------------------------------------------- public functions
@pytest.mark.parametrize("cls", [mx.dgRMatrix, mx.lgRMatrix])
@pytest.mark.parametrize("na_rm", [False, True])
def test_remove_sparse_zeros_csr(gpu, cls, na_rm):
    rng = np.random.default_rng(4)
    p, j, _ = rand_csr(60, 50, 0.2, 8, sorted_cols=False, empty_rows=(3,))
    kind = "d" if cls is mx.dgRMatrix else "l"
    x = values_of(kind, j.size, rng)
    X = cls(p, j, x, (60, 50), [None, [f"c{k}" for k in range(50)]])
    Y = mx.remove_sparse_zeros(X, na_rm)
    keep = ref_keep("csr", kind, x, na_rm)
    assert type(Y) is cls and Y.Dim == X.Dim and Y.Dimnames == X.Dimnames
    np.testing.assert_array_equal(Y.p, ref_indptr(p, keep))
    np.testing.assert_array_equal(Y.j, j[keep])
    same_values(Y.x, x[keep])


def test_remove_sparse_zeros_csc_and_coo(gpu):
    rng = np.random.default_rng(6)
    p, i, _ = rand_csr(30, 40, 0.3, 1)
    x = values_of("d", i.size, rng)
    C = mx.dgCMatrix(p, i, x, (40, 30))
    Y = mx.remove_sparse_zeros(C, True)
    keep = ref_keep("csr", "d", x, True)
    assert type(Y) is mx.dgCMatrix
    np.testing.assert_array_equal(Y.p, ref_indptr(p, keep))
    np.testing.assert_array_equal(Y.i, i[keep])
    same_values(Y.x, x[keep])
    for cls, kind in ((mx.dgTMatrix, "d"), (mx.lgTMatrix, "l")):
        ii, jj = rng.integers(0, 9, 300).astype(np.int32), rng.integers(0, 7, 300).astype(np.int32)
        xx = values_of(kind, 300, rng)
        T = cls(ii, jj, xx, (9, 7))
        for na_rm in (False, True):
            Y = mx.remove_sparse_zeros(T, na_rm)
            keep = ref_keep("coo", kind, xx, na_rm)
            assert type(Y) is cls
            np.testing.assert_array_equal(Y.i, ii[keep])
            np.testing.assert_array_equal(Y.j, jj[keep])
            same_values(Y.x, xx[keep])


def test_remove_sparse_zeros_nothing_removed_shares_arrays(gpu):
    X = mx.dgRMatrix(np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.array([1.0, NA_REAL, 2.0]),
                     (2, 3))
    assert mx.remove_sparse_zeros(X) is X                    # NaN is not removed without na.rm
    Y = mx.remove_sparse_zeros(X, na_rm=True)
    assert Y is not X and Y.x.size == 2


def _r_logical(mk):
    mk = np.asarray(mk)
    if mk.dtype.kind == "f":
        return np.where(np.isnan(mk), NA, (mk != 0)).astype(np.int32)
    return mk.astype(np.int32)


@pytest.mark.parametrize("cls", [mx.dgRMatrix, mx.lgRMatrix, mx.dgCMatrix, mx.dgTMatrix, mx.lgTMatrix])
def test_filterSparse(gpu, cls):
    rng = np.random.default_rng(8)
    kind = "l" if cls in (mx.lgRMatrix, mx.lgTMatrix) else "d"
    coo = cls in (mx.dgTMatrix, mx.lgTMatrix)
    if coo:
        ii, jj = rng.integers(0, 50, 3000).astype(np.int32), rng.integers(0, 40, 3000).astype(np.int32)
        x = values_of(kind, 3000, rng)
        X = cls(ii, jj, x, (50, 40))
    else:
        p, jj, _ = rand_csr(50, 40, 0.4, 12, sorted_cols=False, empty_rows=(5,))
        x = values_of(kind, jj.size, rng)
        X = mx.dgCMatrix(p, jj, x, (40, 50)) if cls is mx.dgCMatrix else cls(p, jj, x, (50, 40))
    masks = [
        (lambda v: v > 0) if kind == "d" else (lambda v: v == 1),                                # callable, bool
        lambda v: np.where(np.arange(v.size) % 3 == 0, np.nan, np.arange(v.size) % 2 * 1.5),   # as.logical(double)
        rng.random(x.size) < 0.5,                                                               # bool vector
        rng.choice(np.array([0, 1, NA], np.int32), size=x.size),                               # R logical with NA
    ]
    for m in masks:
        lg = _r_logical(m(x) if callable(m) else m)
        keep = lg != 0
        want = x[keep].copy()
        want[lg[keep] == NA] = NA_REAL if kind == "d" else NA
        Y = mx.filterSparse(X, m)
        assert type(Y) is cls and Y.Dim == X.Dim
        same_values(Y.x, want)
        if coo:
            np.testing.assert_array_equal(Y.i, X.i[keep])
            np.testing.assert_array_equal(Y.j, X.j[keep])
        else:
            idx, out_idx = (X.i, Y.i) if cls is mx.dgCMatrix else (X.j, Y.j)
            np.testing.assert_array_equal(Y.p, ref_indptr(X.p, keep))
            np.testing.assert_array_equal(out_idx, idx[keep])


# ---------------------------------------------------------------------------------------------- check_sparse_matrix
def test_check_valid_exports_first_failure_order(gpu):
    assert G.check_valid_csr_matrix(np.array([0, 2, 3], np.int32), np.array([0, 4, 1], np.int32), 2, 5) == {}
    cases = [
        (np.array([0, 2, 3], np.int32), [0, -1, 1], "Matrix has negative indices."),
        (np.array([0, 2, 3], np.int32), [0, 5, 1], "Matrix has invalid column indices."),
        (np.array([0, 2, 3], np.int32), [9, NA, 1], "Matrix has negative indices."),      # NA < 0, before >= bound
        (np.array([0, NA, 3], np.int32), [0, 1, 1], "Matrix has missing values in the index pointer."),
        (np.array([0, 3, 2, 3], np.int32), [0, 1, 1], "Matrix index pointer is not monotonicaly increasing."),
        (np.array([0, NA, 2, 3], np.int32), [0, 1, -4], "Matrix has negative indices."),
    ]
    for pp, j, msg in cases:
        assert G.check_valid_csr_matrix(pp, np.array(j, np.int32), pp.size - 1, 5) == {"err": msg}
    assert G.check_valid_csr_matrix(np.zeros(4, np.int32), np.zeros(0, np.int32), 3, 5) == {}   # nnz = 0 passes
    i, j = np.array([0, 3, 1], np.int32), np.array([0, 1, 7], np.int32)
    assert G.check_valid_coo_matrix(i, j, 4, 8) == {}
    assert G.check_valid_coo_matrix(i, j, 3, 8) == {"err": "Matrix has invalid column indices."}
    assert G.check_valid_coo_matrix(i, j, 4, 7) == {"err": "Matrix has invalid column indices."}
    assert G.check_valid_coo_matrix(np.array([0, 9, 1], np.int32), np.array([0, -1, 1], np.int32), 4, 8) == \
        {"err": "Matrix has invalid column indices."}                  # ii is checked before jj
    assert G.check_valid_coo_matrix(i, np.array([0, -1, 1], np.int32), 4, 8) == {"err": "Matrix has negative indices."}
    assert G.check_valid_svec(np.array([1, 3], np.int32), 5) == {}
    assert G.check_valid_svec(np.array([1, 5], np.int32), 5) == {"err": "Matrix has invalid column indices."}  # sic
    assert G.check_valid_svec(np.zeros(0, np.int32), 0) == {}


def test_check_sparse_matrix(gpu):
    X = mx.dgRMatrix(np.array([0, 3, 3, 5], np.int32), np.array([2, 0, 1, 3, 1], np.int32),
                     np.array([1.0, 0.0, 3.0, 4.0, 5.0]), (3, 4))
    j0, x0 = X.j.copy(), X.x.copy()
    Y = mx.check_sparse_matrix(X)                            # zeros removed, then the new arrays sorted
    np.testing.assert_array_equal(Y.p, [0, 2, 2, 4])
    np.testing.assert_array_equal(Y.j, [1, 2, 1, 3])
    same_values(Y.x, np.array([3.0, 1.0, 5.0, 4.0]))
    np.testing.assert_array_equal(X.j, j0)
    same_values(X.x, x0)
    Z = mx.check_sparse_matrix(X, remove_zeros=False)       # nothing removed: sorted copies, X untouched
    np.testing.assert_array_equal(Z.j, [0, 1, 2, 1, 3])
    np.testing.assert_array_equal(X.j, j0)
    C = mx.dgCMatrix(np.array([0, 2, 3], np.int32), np.array([4, 1, 0], np.int32), np.array([1.0, 2.0, 0.0]), (5, 2))
    W = mx.check_sparse_matrix(C)                            # CSC: ncol + 1 pointers, row indices against nrow
    np.testing.assert_array_equal(W.p, [0, 2, 2])
    np.testing.assert_array_equal(W.i, [1, 4])
    T = mx.dgTMatrix(np.array([1, 0], np.int32), np.array([2, 2], np.int32), np.array([0.0, 1.0]), (2, 3))
    np.testing.assert_array_equal(mx.check_sparse_matrix(T, sort=False).i, [0])
    bad = mx.dgRMatrix(np.array([0, 1, 2], np.int32), np.array([0, 4], np.int32), np.array([1.0, 2.0]), (2, 4))
    with pytest.raises(mx.MatrixExtraError, match="Matrix has invalid column indices."):
        mx.check_sparse_matrix(bad)
    bad_c = mx.dgCMatrix(np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32), np.array([1.0, 2.0]), (3, 2))
    with pytest.raises(mx.MatrixExtraError, match="Matrix has invalid column indices."):
        mx.check_sparse_matrix(bad_c)
    badp = mx.dgRMatrix(np.array([0, 2, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0]), (3, 4))
    with pytest.raises(mx.MatrixExtraError, match="not monotonicaly increasing"):
        mx.check_sparse_matrix(badp)


# ---------------------------------------------------------------------------------------------- cfg2 size, device API
@pytest.fixture(scope="module")
def cfg2(gpu):
    p, j, x = synth.csr_fixed(1_000_000, 100_000, 32)
    x = x.copy()
    x[np.random.default_rng(3).random(x.size) < 0.1] = 0.0
    return p, j, x


def test_cfg2_remove_zeros_and_filter(cfg2):
    p, j, x = cfg2
    keep = x != 0
    out = G.remove_zero_valued_csr_numeric(p, j, x, False)
    np.testing.assert_array_equal(out["indptr"], ref_indptr(p, keep))
    np.testing.assert_array_equal(out["indices"], j[keep])
    same_values(out["values"], x[keep])
    Y = mx.filterSparse(mx.dgRMatrix(p, j, x, (1_000_000, 100_000)), lambda v: v > 0.25)
    keep = x > 0.25
    np.testing.assert_array_equal(Y.p, ref_indptr(p, keep))
    np.testing.assert_array_equal(Y.j, j[keep])
    same_values(Y.x, x[keep])


def test_device_csr_remove_zeros_matches_export(cfg2):
    from matrixextra_amd import device as D
    p, j, x = cfg2
    A = D.DeviceCSR.from_host(p, j, x, 100_000)
    R = D.csr_remove_zeros(A)
    out = G.remove_zero_valued_csr_numeric(p, j, x, False)
    hp, hj, hx = R.to_host()
    np.testing.assert_array_equal(hp, out["indptr"])
    np.testing.assert_array_equal(hj, out["indices"])
    same_values(hx, out["values"])
    assert D.csr_remove_zeros(R) is R                         # nothing left to remove
    F = D.csr_filter(A, torch.from_numpy(x > 0.5).cuda())
    keep = x > 0.5
    np.testing.assert_array_equal(F.indptr.cpu().numpy(), ref_indptr(p, keep))
    np.testing.assert_array_equal(F.indices.cpu().numpy(), j[keep])
    lg = torch.from_numpy(np.where(np.arange(x.size) % 2 == 0, NA, 0).astype(np.int32)).cuda()
    L = D.csr_filter(A, lg)                                   # NA keeps the entry with NA_real_ as its value
    assert L.nnz == (x.size + 1) // 2
    np.testing.assert_array_equal(L.values.cpu().numpy().view(np.uint64),
                                  np.full(L.nnz, 0x7FF00000000007A2, np.uint64))
