"""multiply_csr_by_dvec_with_NAs on the device (dvecna.hip) against the numpy model of
dvec_na_model.py: structure exact, every fill cell bit for bit (NA_real_ against the default NaN), stored values bit
for bit under * and /, rtol 1e-13 under ^ %% %/% (the values-only route's own tolerance).  Where the operation itself
makes a NaN, or both operands are NaN, only NaN-ness is compared; every comparison asserts that this covers at most
5 % of the entries, and the main generators keep it at 0."""
import ctypes as C

import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G
from devmem import SLACK, GCsr, GuardedVec
from dvec_na_model import (NA_REAL, OPS, OTHER_NAN, compare, dirty_case, flags, make_csr, make_vector, model, pool,
                           special)

pytestmark = pytest.mark.gpu
OPTION = "mxgpu.dvec_na_route"


def run(p, j, x, v, ncols, op, lhs=True):
    return G.multiply_csr_by_dvec_with_NAs(p, j, x, v, ncols, *flags(op), lhs)


def check(p, j, x, v, ncols, op):
    p0, j0, x0, v0 = p.copy(), j.copy(), x.copy(), np.array(v, dtype=np.float64)
    exp = model(p, j, x, v, ncols, op)
    got = run(p, j, x, v, ncols, op)
    share = compare(got, exp, op)
    assert np.array_equal(p, p0) and np.array_equal(j, j0)
    assert np.array_equal(x.view(np.uint64), x0.view(np.uint64))
    assert np.array_equal(np.asarray(v, dtype=np.float64).view(np.uint64), v0.view(np.uint64))
    return got, exp, share


# ---- regime A: the vector's length divides the number of rows ----------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 300])
@pytest.mark.parametrize("op", OPS)
def test_row_ruled(gpu, op, m):
    lengths = {1: [1], 7: [1, 7], 300: [1, 25, 300]}[m]
    for ncols in (1, 63, 64, 65, 200):
        empty = (0, m - 1) if m > 2 else ()
        full = (1, m // 2) if m > 2 else (0,)
        p, j, x = make_csr(m, ncols, 0.2, 11 * m + ncols, empty_rows=empty, full_rows=full, positive=op == "^")
        for L in lengths:
            # specials first, last and adjacent (rows 0 and 1; row 1 is a full row inside a filled row)
            v = make_vector(L, op, L + ncols, at=(0, 1, L - 1))
            got, exp, share = check(p, j, x, v, ncols, op)
            assert share == 0 and (exp["fill"].any() or m == 1)          # m == 1: the one row is a full one
            if L > 1:
                assert (np.diff(exp["indptr"]) == ncols).sum() >= 2      # filled rows
        if m > 1:
            v = make_vector(m, op, 5, share=0.0)                          # nothing special: every row plain
            got, exp, _ = check(p, j, x, v, ncols, op)
            assert np.array_equal(got["indptr"], p) and not exp["fill"].any()


@pytest.mark.parametrize("op", OPS)
def test_row_ruled_every_special_value(gpu, op):
    m, ncols = 24, 70
    p, j, x = make_csr(m, ncols, 0.3, 4, empty_rows=(3,), full_rows=(2,), positive=op == "^")
    vals = pool(op) + [np.inf, -np.inf, 0.0, -1.5, 2.0, NA_REAL, OTHER_NAN, 1.0]
    v = np.array((vals * 3)[:m])
    check(p, j, x, v, ncols, op)
    check(p, j, x, v[:12], ncols, op)


@pytest.mark.parametrize("avg,G_want", [(2, 4), (7, 8), (14, 16), (28, 32), (60, 64)])
def test_row_ruled_lane_groups_in_guarded_buffers(gpu, avg, G_want):
    """the device-level pair at every lane-group width the dispatcher offers, operands and outputs between guards"""
    lib = _lib.load()
    m, ncols, L, op = 300, 200, 25, "/"
    p, j, x = make_csr(m, ncols, avg / ncols, 100 + avg, empty_rows=(0, 299), full_rows=(26,))
    v = make_vector(L, op, 3, at=(0, 1, L - 1))
    exp = model(p, j, x, v, ncols, op)
    A, gv = GCsr(p, j, x), GuardedVec(np.float64, data=v)
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_by_dvec_na_rows_workspace_bytes(m))
    gp, total = GuardedVec(np.int32, n=m + 1), C.c_int64(-1)
    code = C.c_int(_lib.MX_DV_OPS[op])
    _lib.check(lib.mxd_csr_by_dvec_na_rows_count(C.c_int(m), C.c_int(ncols), C.c_int64(A.nnz), A.p.ptr, gv.ptr,
                                                 C.c_int64(L), code, gws.ptr, gp.ptr, C.byref(total), None))
    nout = int(total.value)
    assert nout == exp["indices"].size
    indptr = gp.result()
    gws._download()
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(np.float64, n=nout + SLACK)
    _lib.check(lib.mxd_csr_by_dvec_na_rows_fill(C.c_int(m), C.c_int(ncols), C.c_int64(A.nnz), A.p.ptr, A.j.ptr, A.xptr,
                                                gv.ptr, C.c_int64(L), code, gp.ptr, gj.ptr, gx.ptr, None))
    _lib.check(lib.mx_stream_sync(None))
    assert _lib.last_row_launch() == ("mxd_csr_by_dvec_na_rows_fill", G_want)
    A.assert_untouched()
    gv.assert_untouched()
    compare(dict(indptr=indptr, indices=gj.result(nout), values=gx.result(nout)), exp, op)
    # the export picks the same width
    run(p, j, x, v, ncols, op)
    assert _lib.last_row_launch() == ("mxd_csr_by_dvec_na_rows_fill", G_want)


# ---- regime B: every other length --------------------------------------------------------------------------------
FLAT = [(7, 5, 3), (7, 5, 10), (7, 5, 14), (7, 5, 35), (300, 130, 77), (300, 130, 601), (300, 130, 39000)]


@pytest.mark.parametrize("m,ncols,L", FLAT)
@pytest.mark.parametrize("op", OPS)
def test_flat(gpu, op, m, ncols, L):
    N = m * ncols
    p, j, x = make_csr(m, ncols, 0.25, m + L, empty_rows=(0, m - 1), positive=op == "^")
    # specials at position 0 (its first cell is in the empty row 0), at L - 1, and at the one that hits cell N - 1
    share = 0.3 if L < 100 else 0.02
    v = make_vector(L, op, L, at=(0, L - 1, (N - 1) % L), share=share)
    got, exp, ex = check(p, j, x, v, ncols, op)
    assert ex == 0 and not exp["alias"]
    assert 0 < exp["new"] < exp["candidates"]                     # some special cells fall on stored ones
    d = np.diff(exp["indptr"]) - np.diff(p)
    assert d[0] > 0                                                 # an empty row receives entries
    assert got["indices"][-1] == ncols - 1 or ((N - 1) % m != m - 1)
    if m == 300:                                                    # new entries before the first / after the last stored
        rows_of = np.repeat(np.arange(m), np.diff(exp["indptr"]))
        first_new = exp["fill"][exp["indptr"][:-1][d > 0]]
        last_new = exp["fill"][exp["indptr"][1:][d > 0] - 1]
        assert first_new.any() and last_new.any() and rows_of.size == got["indices"].size
    classes = set(np.ascontiguousarray(exp["values"][exp["fill"]]).view(np.uint64).tolist())
    assert len(classes) >= (4 if op == "^" and L >= 14 else 2)     # NaN and NA_real_; for ^ also 1 and +Inf


def test_flat_last_cell(gpu):
    """a special position whose last repeat is exactly flat cell N - 1, in the last row and column"""
    m, ncols, L = 7, 5, 10
    p, j, x = make_csr(m, ncols, 0.2, 1, empty_rows=(6,))
    v = np.ones(L)
    v[(m * ncols - 1) % L] = NA_REAL
    got, exp, _ = check(p, j, x, v, ncols, "*")
    assert got["indices"][-1] == ncols - 1 and got["indptr"][-1] - got["indptr"][-2] >= 1


@pytest.mark.parametrize("op", ["*", "/", "%/%"])
def test_flat_no_new_entry_returns_the_input_structure(gpu, op):
    m, ncols = 7, 5
    p, j, x = make_csr(m, ncols, 1.0, 2, positive=True)              # every cell stored
    v = make_vector(3, op, 1, at=(1,), share=0.0)
    assert special(op, v).any()
    got = run(p, j, x, v, ncols, op)
    assert got["indptr"] is p and got["indices"] is j
    exp = model(p, j, x, v, ncols, op)
    assert exp["alias"]
    compare(got, exp, op)
    # a vector without anything special, should a caller send one
    got = run(p, j, x, np.array([1.0, 2.0, 4.0]), ncols, op)
    assert got["indptr"] is p and got["indices"] is j


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("op", ["*", "/"])
def test_dirty_matrix_stays_under_the_cap(gpu, op, flat):
    """NaN / Inf / 0 inside X: the operation makes NaNs of its own, compared by NaN-ness, at most 5 % of the entries"""
    p, j, x, v, ncols = dirty_case(op, flat)
    got, exp, share = check(p, j, x, v, ncols, op)
    assert 0 < share <= 0.05


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_overflow_is_refused_before_the_result_exists(gpu):
    m, ncols = 70001, 70000
    p, j, x = np.zeros(m + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)
    with pytest.raises(_lib.MxError, match=r"Error: the resulting matrix would have too many entries for a sparse CSR "
                                           r"representation \(int overflow\)\."):
        run(p, j, x, np.zeros(2), ncols, "/")                       # flat: 4.9e9 candidate cells
    with pytest.raises(_lib.MxError, match="exceeds R's int32 index range"):
        run(p, j, x, np.zeros(1), ncols, "/")                       # row-ruled: 70001 rows of 70000 columns


def test_export_refusals(gpu):
    p, j, x = make_csr(6, 4, 0.5, 1)
    for op in ("^", "/", "%%"):
        with pytest.raises(_lib.MxError, match="Internal error"):
            run(p, j, x, np.array([0.0, 1.0]), 4, op, lhs=False)
    with pytest.raises(_lib.MxError, match="Internal error"):
        G.multiply_csr_by_dvec_with_NAs(p, j, x, np.array([0.0, 1.0]), 4, False, False, False, False, False, True)
    with pytest.raises(_lib.MxError, match="more entries than the matrix"):
        run(p, j, x, np.zeros(25), 4, "/")
    # * and %/% go through with X on the right; %/% is applied with X on the left, as the reference does
    v = np.array([NA_REAL, 2.0, 0.0])
    compare(run(p, j, x, v, 4, "*", lhs=False), model(p, j, x, v, 4, "*", False), "*")
    compare(run(p, j, x, v, 4, "%/%", lhs=False), model(p, j, x, v, 4, "%/%", False), "%/%")


# ---- the other layers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [25, 77])
@pytest.mark.parametrize("op", ["*", "^", "%%"])
def test_device_layer_matches_the_export(gpu, op, L):
    import torch
    from matrixextra_amd import device as D
    m, ncols = 300, 130
    p, j, x = make_csr(m, ncols, 0.1, 8, empty_rows=(0,), positive=op == "^")
    v = make_vector(L, op, 2, at=(0, L - 1), share=0.1)
    want = run(p, j, x, v, ncols, op)
    dev = torch.device("cuda")
    A = D.DeviceCSR(torch.from_numpy(p).to(dev), torch.from_numpy(j).to(dev), torch.from_numpy(x).to(dev), m, ncols,
                    int(j.size))
    dp, dj, dx = D.csr_by_dvec_keep_na(A, torch.from_numpy(v).to(dev), op)
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy(), want["indptr"]) and np.array_equal(dj.cpu().numpy(), want["indices"])
    assert np.array_equal(dx.cpu().numpy().view(np.uint64), want["values"].view(np.uint64))
    assert np.array_equal(A.indices.cpu().numpy(), j) and np.array_equal(A.values.cpu().numpy(), x)
    if L == 77:
        ones = torch.ones(L, dtype=torch.float64, device=dev)
        sp, sj, _ = D.csr_by_dvec_keep_na(A, ones, op)
        assert sp is A.indptr and sj is A.indices


def test_operators_with_the_option(gpu, monkeypatch):
    p, j, x = make_csr(12, 9, 0.3, 6, empty_rows=(2,))
    X = mx.dgRMatrix(p, j.copy(), x, (12, 9), [None, list("abcdefghi")])
    v = np.array([2.0, 0.0, 4.0, -1.0])
    with pytest.raises(mx.MatrixExtraError, match="981-1131"):
        X / v                                                       # the option is not set
    T = mx.as_coo_matrix(X)
    w = np.array([1.0, NA_REAL, 3.0, np.inf, 2.0])
    with pytest.raises(mx.MatrixExtraError, match="981-1131"):
        T * w
    monkeypatch.setitem(mx.options, OPTION, True)
    j0, x0, ti, tj = X.j.copy(), X.x.copy(), T.i.copy(), T.j.copy()
    out = X / v
    assert type(out) is mx.dgRMatrix and tuple(out.Dim) == (12, 9) and out.Dimnames[1] == list("abcdefghi")
    compare(dict(indptr=out.p, indices=out.j, values=out.x), model(p, j, x, v, 9, "/"), "/")
    with pytest.warns(UserWarning, match="not a multiple of matrix dimension"):
        out = T * w
    assert type(out) is mx.dgRMatrix and tuple(out.Dim) == (12, 9)
    compare(dict(indptr=out.p, indices=out.j, values=out.x), model(p, j, x, w, 9, "*"), "*")
    assert np.array_equal(X.j, j0) and np.array_equal(X.x, x0) and np.array_equal(T.i, ti) and np.array_equal(T.j, tj)
