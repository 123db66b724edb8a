"""Device level of the reduction family (mxd_segment_reduce, mxd_csr_column_order, mxd_csr_diag) on guarded buffers
(tests/devmem.py): every operand and output lies between sentinels, outputs and the workspace start as poison, inputs
are checked untouched.  Expectations come from tests/reduce_model.py: exact data is compared with `==`, general floats
within the any-order summation bound derived there, and every call is repeated and must return the same bits.  The
shapes are the smallest at which a reduction tiled by 4096 entries can go wrong."""
import numpy as np
import pytest

import reduce_model as RM
from conftest import rand_csr
from devmem import GCsr, GuardedVec, _sync
from matrixextra_amd import _lib

pytestmark = pytest.mark.gpu

CASES = RM.segment_cases()
VD = {"d": _lib.MX_F64, "l": _lib.MX_LGL, "n": _lib.MX_NONE}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def dev_segment_reduce(op, values, kind, perm, segptr, nnz, na_rm):
    """one mxd_segment_reduce on guarded buffers: (out, skipped)"""
    lib = _lib.load()
    nseg = segptr.size - 1
    gv = None if values is None else GuardedVec(values.dtype, data=values)
    gperm = None if perm is None else GuardedVec(np.int32, data=perm)
    gseg = GuardedVec(np.int32, data=segptr)
    gout, gskip = GuardedVec(np.float64, n=nseg), GuardedVec(np.int32, n=nseg)
    gws = GuardedVec(np.uint8, n=4 * lib.mxd_compact_workspace_bytes(nnz))
    _lib.check(lib.mxd_segment_reduce(op, None if gv is None else gv.ptr, VD[kind], None if gperm is None else gperm.ptr,
                                      nnz, gseg.ptr, nseg, int(na_rm), gout.ptr, gskip.ptr, gws.ptr, None))
    _sync()
    for g in (gv, gperm, gseg):
        if g is not None:
            g.assert_untouched()
    gws._download()                                      # the guards around the workspace
    return gout.result(), gskip.result()                 # every segment written, nothing behind them


@pytest.mark.parametrize("flavour", RM.FLAVOURS)
@pytest.mark.parametrize("name", list(CASES))
def test_segment_reduce(gpu, name, flavour):
    segptr = CASES[name]
    nnz = int(segptr[-1])
    values, kind = RM.case_values(name, nnz, flavour)
    f = RM.as_f64(values, kind, nnz)
    exact = flavour in ("exact", "logical", "pattern")
    perms = [None, np.random.default_rng(nnz + 1).permutation(nnz).astype(np.int32)]
    for perm in perms:
        for na_rm in (False, True):
            for op in RM.OPS:
                what = f"{name} / {flavour} / {RM.OP_NAMES[op]} / perm {perm is not None} / na_rm {na_rm}"
                want, want_skipped, bound = RM.segment_reduce(op, f, segptr, perm, na_rm)
                got, skipped = dev_segment_reduce(op, values, kind, perm, segptr, nnz, na_rm)
                RM.assert_reduced(got, skipped, want, want_skipped, np.zeros_like(bound) if exact else bound, what)
                again, skipped2 = dev_segment_reduce(op, values, kind, perm, segptr, nnz, na_rm)
                assert np.array_equal(bits(got), bits(again)) and np.array_equal(skipped, skipped2), \
                    f"{what}: a repeated call gave other bits"


def test_a_nan_inside_a_segment_surfaces_from_abs_max(gpu):
    """fmax would drop it: one NaN in the middle of a three-tile segment, at a tile edge, and as a segment's only entry"""
    segptr = CASES["three-tile-segment-between-empties"]
    nnz = int(segptr[-1])
    for q in (3 + 5000, RM.TILE - 1, RM.TILE, 10003):
        v = np.arange(1.0, nnz + 1.0)
        v[q] = np.nan
        got, _ = dev_segment_reduce(RM.ABS_MAX, v, "d", None, segptr, nnz, False)
        want = RM.segment_reduce(RM.ABS_MAX, v, segptr)[0]
        assert np.isnan(want).sum() == 1
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
        got, skipped = dev_segment_reduce(RM.ABS_MAX, v, "d", None, segptr, nnz, True)
        want, want_skipped, _ = RM.segment_reduce(RM.ABS_MAX, v, segptr, None, True)
        assert np.array_equal(got, want) and np.array_equal(skipped, want_skipped) and skipped.sum() == 1


# ---- column order ---------------------------------------------------------------------------------------------------------
def order_cases():
    def dense_first(m, n, seed):
        p, j, _ = rand_csr(m, n - 1, 0.02, seed)
        rows = np.repeat(np.arange(m), np.diff(p))
        jj = np.concatenate([np.zeros(m, dtype=np.int32), j + 1])
        rr = np.concatenate([np.arange(m), rows])
        o = np.lexsort((jj, rr))
        pp = np.zeros(m + 1, dtype=np.int32)
        pp[1:] = np.cumsum(np.bincount(rr, minlength=m))
        return pp, jj[o].astype(np.int32)

    out = {}
    p, j, _ = rand_csr(300, 70, 0.2, 5, sorted_cols=False)
    out["300x70-unsorted"] = (p, j, 300, 70)
    p, j, _ = rand_csr(500, 1, 0.5, 6)
    out["one-column"] = (p, j, 500, 1)
    p, j, _ = rand_csr(60, 257, 0.3, 7, sorted_cols=False)
    out["257-columns-second-digit"] = (p, j, 60, 257)
    p, j = dense_first(9000, 40, 8)
    out["9000x40-dense-first-column"] = (p, j, 9000, 40)
    p, j, _ = rand_csr(200, 30, 0.3, 9)
    out["empty-columns-at-both-ends"] = (p, (j + 5).astype(np.int32), 200, 40)
    out["no-entries"] = (np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), 3, 6)
    return out


ORDER_CASES = order_cases()


def dev_column_order(p, j, m, n):
    lib = _lib.load()
    A = GCsr(p, j)
    nnz = int(j.size)
    gperm, gcolptr = GuardedVec(np.int32, n=nnz), GuardedVec(np.int32, n=n + 1)
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_transpose_workspace_bytes(nnz))
    rc = lib.mxd_csr_column_order(m, n, A.p.ptr, A.j.ptr, nnz, gperm.ptr, gcolptr.ptr, gws.ptr, None)
    err = None if rc == 0 else lib.mx_last_error().decode()
    _sync()
    A.assert_untouched()
    gws._download()
    return gperm, gcolptr, err


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_column_order(gpu, name):
    p, j, m, n = ORDER_CASES[name]
    if name == "9000x40-dense-first-column":
        assert np.count_nonzero(j == 0) == 9000 > 2 * RM.TILE          # that column spans three tiles
    if name == "empty-columns-at-both-ends":
        assert j.min() >= 5 and j.max() < 35
    want_perm, want_colptr = RM.column_order(j, n)
    gperm, gcolptr, err = dev_column_order(p, j, m, n)
    assert err is None
    perm, colptr = gperm.result(), gcolptr.result()
    assert np.array_equal(perm, want_perm) and np.array_equal(perm, np.argsort(j, kind="stable"))
    assert np.array_equal(colptr, want_colptr)
    again = dev_column_order(p, j, m, n)
    assert np.array_equal(again[0].result(), perm) and np.array_equal(again[1].result(), colptr)


def test_column_order_refuses_an_index_out_of_range(gpu):
    p, j, m, n = ORDER_CASES["300x70-unsorted"]
    for bad in (70, -1, 2 ** 31 - 1):
        jj = j.copy()
        jj[jj.size // 2] = bad
        gperm, gcolptr, err = dev_column_order(p, jj, m, n)
        assert err is not None and "column index outside [0, 70)" in err
        gperm._download()                                # what it wrote stayed between the guards
        gcolptr._download()


def test_column_sums_through_the_order(gpu):
    """the order feeds the reduction: column sums of the dense-first-column case, exact data"""
    p, j, m, n = ORDER_CASES["9000x40-dense-first-column"]
    x = np.random.default_rng(11).integers(-9, 10, size=j.size).astype(np.float64)
    gperm, gcolptr, err = dev_column_order(p, j, m, n)
    assert err is None
    perm, colptr = gperm.result(), gcolptr.result()
    got, _ = dev_segment_reduce(RM.SUM, x, "d", perm, colptr, j.size, False)
    want = np.zeros(n)
    np.add.at(want, j, x)
    assert np.array_equal(got, want)


# ---- diag -----------------------------------------------------------------------------------------------------------------
def diag_case(m, n, sorted_cols, kind, seed):
    """every row kind: an empty row (3), a row whose only entry is the diagonal (5), rows with and without one"""
    p, j, x = rand_csr(m, n, 0.25, seed, sorted_cols=sorted_cols, dtype=kind, empty_rows=(3, 5))
    rows = np.repeat(np.arange(m), np.diff(p))
    at = int(p[5])
    j = np.insert(j, at, 5).astype(np.int32)
    if x is not None:
        x = np.insert(x, at, -2.5 if kind == "d" else RM.NA_LOGICAL).astype(x.dtype)
    p = p.copy()
    p[6:] += 1
    assert p[4] == p[3] and p[6] - p[5] == 1 and rows.size + 1 == j.size
    return p, j, x


@pytest.mark.parametrize("kind", ["d", "l", "n"])
@pytest.mark.parametrize("sorted_cols", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("shape", [(50, 80), (80, 50)], ids=["50x80", "80x50"])
def test_diag(gpu, shape, sorted_cols, kind):
    lib = _lib.load()
    m, n = shape
    p, j, x = diag_case(m, n, sorted_cols, kind, seed=m + (7 if sorted_cols else 0))
    want = RM.diag(p, j, x, kind, m, n)
    assert want[3] == 0 and want[5] == (-2.5 if kind == "d" else RM.NA_LOGICAL if kind == "l" else 1)
    assert np.count_nonzero(want) > 5 and np.count_nonzero(want == 0) > 5
    A = GCsr(p, j, x)
    for rows_sorted in ([0, 1] if sorted_cols else [0]):               # the scan serves any rows, the search sorted ones
        gout = GuardedVec(np.float64 if kind == "d" else np.int32, n=min(m, n))
        _lib.check(lib.mxd_csr_diag(m, n, A.p.ptr, A.j.ptr, A.xptr, VD[kind], j.size, rows_sorted, gout.ptr, None))
        _sync()
        A.assert_untouched()
        assert np.array_equal(gout.result(), want), f"rows_sorted {rows_sorted}"


def test_diag_takes_the_first_of_repeated_entries(gpu):
    lib = _lib.load()
    p = np.array([0, 3, 6], dtype=np.int32)
    j = np.array([1, 0, 0, 1, 1, 0], dtype=np.int32)
    x = np.array([9.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    A = GCsr(p, j, x)
    gout = GuardedVec(np.float64, n=2)
    _lib.check(lib.mxd_csr_diag(2, 2, A.p.ptr, A.j.ptr, A.xptr, _lib.MX_F64, 6, 0, gout.ptr, None))
    _sync()
    assert np.array_equal(gout.result(), [4.0, 6.0]) and np.array_equal(RM.diag(p, j, x, "d", 2, 2), [4.0, 6.0])
