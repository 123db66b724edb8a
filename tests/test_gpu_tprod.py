"""Device level of the transposed products (mxd_segment_dot, mxd_csr_transpose_by_order) on guarded buffers
(tests/devmem.py): every operand and output lies between sentinels, outputs and the workspace start as poison, inputs
are checked untouched.  The oracle of the segmented dot is reduce_model.segment_reduce over the written-out products
(tests/tprod_model.py): exact data is compared with `==`, general floats within that function's any-order bound, and
results that are not finite by their class.  Beyond that the dot must equal, bit for bit, mxd_segment_reduce(MX_RED_SUM)
over the uploaded products: a product fused into the addition behind it would differ there.  Every call is repeated and
must return the same bits.  The transpose by a column order is compared with mxd_csr_transpose array for array."""
import numpy as np
import pytest

import reduce_model as RM
import tprod_model as TM
from conftest import rand_csr
from devmem import GCsr, GuardedVec, _sync, dev_csr_transpose, value_dtype_of
from matrixextra_amd import _lib

pytestmark = pytest.mark.gpu

SEGMENT_CASES = RM.segment_cases()
PATTERN_CASES = TM.pattern_cases()
NW = 97                                                  # length of w for the cases that are a segptr alone


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _ptr(g):
    return None if g is None else g.ptr


def dev_segment_dot(x, perm, key, w, segptr, nnz):
    """one mxd_segment_dot on guarded buffers: out"""
    lib = _lib.load()
    nseg = segptr.size - 1
    gx = None if x is None else GuardedVec(np.float64, data=x)
    gperm = None if perm is None else GuardedVec(np.int32, data=perm)
    gkey, gw, gseg = GuardedVec(np.int32, data=key), GuardedVec(np.float64, data=w), GuardedVec(np.int32, data=segptr)
    gout = GuardedVec(np.float64, n=nseg)
    gws = GuardedVec(np.uint8, n=4 * lib.mxd_compact_workspace_bytes(nnz))
    _lib.check(lib.mxd_segment_dot(_ptr(gx), _lib.MX_NONE if x is None else _lib.MX_F64, _ptr(gperm), gkey.ptr, gw.ptr,
                                   w.size, nnz, gseg.ptr, nseg, gout.ptr, gws.ptr, None))
    _sync()
    for g in (gx, gperm, gkey, gw, gseg):
        if g is not None:
            g.assert_untouched()
    gws._download()                                      # the guards around the workspace
    return gout.result()                                 # every segment written, nothing behind them


def dev_segment_sum(t, perm, segptr, nnz):
    """mxd_segment_reduce(MX_RED_SUM) over the uploaded products"""
    lib = _lib.load()
    nseg = segptr.size - 1
    gt, gseg = GuardedVec(np.float64, data=t), GuardedVec(np.int32, data=segptr)
    gperm = None if perm is None else GuardedVec(np.int32, data=perm)
    gout = GuardedVec(np.float64, n=nseg)
    gws = GuardedVec(np.uint8, n=4 * lib.mxd_compact_workspace_bytes(nnz))
    _lib.check(lib.mxd_segment_reduce(RM.SUM, gt.ptr, _lib.MX_F64, _ptr(gperm), nnz, gseg.ptr, nseg, 0, gout.ptr, None,
                                      gws.ptr, None))
    _sync()
    return gout.result()


def check_dot(what, flavour, x, perm, key, w, segptr):
    nnz = int(key.size)
    t = TM.terms(x, perm, key, w)
    got = dev_segment_dot(x, perm, key, w, segptr, nnz)
    want, _, bound = RM.segment_reduce(RM.SUM, t, segptr)
    if flavour == "exact":
        exact = np.zeros(segptr.size - 1)
        np.add.at(exact, np.repeat(np.arange(segptr.size - 1), np.diff(segptr)), t)
        assert np.array_equal(got, exact), f"{what}: differs from numpy on exact data"
        bound = np.zeros_like(bound)
    RM.assert_reduced(got, None, want, None, bound, what)
    if flavour.startswith("special") and nnz > 1:
        assert not np.isfinite(want).all(), f"{what}: the case has no result that is not finite"
    again = dev_segment_dot(x, perm, key, w, segptr, nnz)
    assert np.array_equal(bits(got), bits(again)), f"{what}: a repeated call gave other bits"
    if not flavour.startswith("special"):               # the FMA guard: the same bits as the sum of the written-out products
        by_sum = dev_segment_sum(TM.in_storage_order(t, perm), perm, segptr, nnz)
        assert np.array_equal(bits(got), bits(by_sum)), f"{what}: not the bits of mxd_segment_reduce over the products"


@pytest.mark.parametrize("flavour", TM.FLAVOURS)
@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_segment_dot_over_the_reduction_cases(gpu, name, flavour):
    segptr = SEGMENT_CASES[name]
    nnz = int(segptr[-1])
    rng = np.random.default_rng(nnz + 3)
    key = rng.integers(0, NW, size=nnz).astype(np.int32)
    for perm in (None, rng.permutation(nnz).astype(np.int32)):
        x, w = TM.operands(name, nnz, NW, flavour, perm, key)
        check_dot(f"{name} / {flavour} / perm {perm is not None}", flavour, x, perm, key, w, segptr)


@pytest.mark.parametrize("flavour", TM.FLAVOURS)
@pytest.mark.parametrize("form", ["column", "row"])
@pytest.mark.parametrize("name", list(PATTERN_CASES))
def test_segment_dot_over_the_pattern_cases(gpu, name, form, flavour):
    p, j, m, K = PATTERN_CASES[name]
    perm, key, segptr, nw = (TM.column_form if form == "column" else TM.row_form)(p, j, K)
    x, w = TM.operands(name, int(j.size), nw, flavour, perm, key)
    check_dot(f"{name} / {form} / {flavour}", flavour, x, perm, key, w, segptr)


def test_the_pattern_cases_are_what_they_are_named():
    for name, (p, j, m, K) in PATTERN_CASES.items():
        assert p.size == m + 1 and p[-1] == j.size and (j.size == 0 or (j.min() >= 0 and j.max() < K)), name
        rows = TM.rows_of_entries(p)
        if j.size >= 2:
            cells = rows.astype(np.int64) * K + j
            assert np.unique(cells).size < cells.size, f"{name}: no repeated cell"
        if j.size > 300 and K > 1:
            assert any(np.any(np.diff(j[p[r]:p[r + 1]]) < 0) for r in range(m)), f"{name}: every row is sorted"
    assert [int(PATTERN_CASES[f"nnz-{n}"][1].size) for n in (0, 1, 4095, 4096, 4097)] == [0, 1, 4095, 4096, 4097]
    p, j, m, K = PATTERN_CASES["column-ends-on-the-tile-edge"]
    assert RM.column_order(j, K)[1][1] == RM.TILE
    p, j, m, K = PATTERN_CASES["empty-columns-and-rows-at-both-ends"]
    assert j.min() >= 5 and j.max() < 35 and p[20] == 0 and p[180] == p[200]
    p, j, m, K = PATTERN_CASES["9000x40-dense-first-column"]
    assert np.count_nonzero(j == 0) == 9000 > 2 * RM.TILE and 0.015 < np.count_nonzero(j) / (9000 * 39) < 0.025


def test_positions_out_of_range_read_element_zero(gpu):
    """rd_tile_kernel's rule: a bad perm or key value is replaced by 0 before it is used"""
    p, j, m, K = PATTERN_CASES["nnz-4097"]
    perm, key, segptr, nw = TM.column_form(p, j, K)
    x, w = TM.operands("bad", int(j.size), nw, "exact", perm, key)
    bad_perm, bad_key = perm.copy(), key.copy()
    for q, v in ((5, -1), (RM.TILE, j.size), (RM.TILE - 2, 2 ** 31 - 1)):
        bad_perm[q] = v
    for q, v in ((7, -3), (RM.TILE - 1, nw), (j.size - 1, 2 ** 31 - 1)):
        bad_key[q] = v
    fixed_perm = np.where((bad_perm < 0) | (bad_perm >= j.size), 0, bad_perm).astype(np.int32)
    fixed_key = np.where((bad_key < 0) | (bad_key >= nw), 0, bad_key).astype(np.int32)

    def exact(pm, ky):
        out = np.zeros(segptr.size - 1)
        np.add.at(out, np.repeat(np.arange(segptr.size - 1), np.diff(segptr)), TM.terms(x, pm, ky, w))
        return out

    assert not np.array_equal(exact(fixed_perm, fixed_key), exact(perm, key))       # the replacements show
    got = dev_segment_dot(x, bad_perm, bad_key, w, segptr, int(j.size))
    assert np.array_equal(got, exact(fixed_perm, fixed_key))


# ---- the transpose by a column order --------------------------------------------------------------------------------------
def order_cases():
    """the column-order cases of tests/test_gpu_reduce.py, rebuilt here"""
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


def dev_order(A, m, n):
    lib = _lib.load()
    gperm, gcolptr = GuardedVec(np.int32, n=A.nnz), GuardedVec(np.int32, n=n + 1)
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_transpose_workspace_bytes(A.nnz))
    _lib.check(lib.mxd_csr_column_order(m, n, A.p.ptr, A.j.ptr, A.nnz, gperm.ptr, gcolptr.ptr, gws.ptr, None))
    _sync()
    return gperm, gcolptr


def dev_by_order(A, m, x, gperm, rows=True, values=True, value_dtype=None):
    """one mxd_csr_transpose_by_order: (out_rows, out_values) as GuardedVecs, None for a null output"""
    lib = _lib.load()
    vd = value_dtype_of(x) if value_dtype is None else value_dtype
    grows = GuardedVec(np.int32, n=A.nnz) if rows else None
    gvals = GuardedVec(np.float64 if x is None else x.dtype, n=A.nnz) if values else None
    _lib.check(lib.mxd_csr_transpose_by_order(m, A.nnz, A.p.ptr, A.xptr, vd, gperm.ptr, _ptr(grows), _ptr(gvals), None))
    _sync()
    A.assert_untouched()
    gperm._download()                                    # an output of the order: its guards
    return grows, gvals


@pytest.mark.parametrize("kind", ["d", "l"])
@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_transpose_by_order_equals_the_transpose(gpu, name, kind):
    p, j, m, n = ORDER_CASES[name]
    rng = np.random.default_rng(len(name))
    if kind == "d":
        x = rng.normal(size=j.size)
        x[::7] = np.nan
        x[1::11] = -0.0
    else:
        x = rng.choice(np.array([0, 1, RM.NA_LOGICAL], dtype=np.int32), size=j.size, p=[0.2, 0.6, 0.2])
    want_p, want_j, want_x = dev_csr_transpose(p, j, x, n)
    assert want_j.size == j.size                         # no repeated cells: nothing was merged
    A = GCsr(p, j, x)
    gperm, gcolptr = dev_order(A, m, n)
    colptr = gcolptr.result()
    grows, gvals = dev_by_order(A, m, x, gperm)
    rows, vals = grows.result(), gvals.result()
    assert np.array_equal(colptr, want_p) and np.array_equal(rows, want_j)
    assert np.array_equal(bits(vals), bits(want_x))
    # the null-output forms: each output alone is the same array, and neither is no call at all
    only_rows, none = dev_by_order(A, m, x, gperm, values=False)
    assert none is None and np.array_equal(only_rows.result(), rows)
    none, only_vals = dev_by_order(A, m, x, gperm, rows=False)
    assert none is None and np.array_equal(bits(only_vals.result()), bits(vals))
    assert dev_by_order(A, m, x, gperm, rows=False, values=False) == (None, None)
    # a pattern: the values buffer is not written even when one is given
    pat_rows, pat_vals = dev_by_order(A, m, x, gperm, value_dtype=_lib.MX_NONE)
    assert np.array_equal(pat_rows.result(), rows)
    pat_vals.result(written=0)
