"""The COO sort on the device (mxd_coo_sort, csrc/transpose.hip) and every layer above it.

Device level: the triplets, the values and the workspace sit in guarded buffers (tests/devmem.py), so a store outside
an operand shows.  Shapes are the smallest at which the passes can go wrong: the tile edges, one / two / three radix
passes on each key, a single row or column, reversed and sorted input, repeated cells.  Every comparison is exact
(the routine only moves data): against the stable numpy model of tests/coo_sort_model.py, and at the export level
against the reference-run fixture tests/golden/coo_sort_golden.npz under that module's bars."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import coo_sort_model as CM
import matrixextra_amd as mx
from devmem import GuardedVec, _sync
from matrixextra_amd import _lib, exports as G, matrices

pytestmark = pytest.mark.gpu

VD = {"numeric": _lib.MX_F64, "logical": _lib.MX_LGL, "binary": _lib.MX_NONE}


def _tile():
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "transpose.hip")).read()
    block = int(re.search(r"constexpr int TP_BLOCK = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int TP_ITEMS = (\d+);", src).group(1))
    assert re.search(r"constexpr int TP_TILE = TP_BLOCK \* TP_ITEMS;", src)
    return block * items


TP_TILE = _tile()
RECORDS, _META = CM.load()


def dev_coo_sort(i, j, x, kind):
    """mxd_coo_sort on guarded operands: (return code, was_sorted, the three guarded vectors)"""
    lib = _lib.load()
    n = int(i.size)
    gi, gj = GuardedVec(np.int32, data=i), GuardedVec(np.int32, data=j)
    gx = None if x is None else GuardedVec(x.dtype, data=x)
    gws = GuardedVec(np.uint8, n=lib.mxd_coo_sort_workspace_bytes(n))
    was = C.c_int(-1)
    rc = lib.mxd_coo_sort(gi.ptr, gj.ptr, None if gx is None else gx.ptr, n, VD[kind], gws.ptr, C.byref(was), None)
    _sync()
    gws._download()                                                 # the guards around the workspace are intact
    return rc, was.value, (gi, gj, gx)


def sorted_on_device(i, j, x, kind, expect_sorted=False):
    rc, was, (gi, gj, gx) = dev_coo_sort(i, j, x, kind)
    assert rc == 0, _lib.load().mx_last_error().decode()
    assert was == int(expect_sorted)
    if expect_sorted:                                               # nothing is written, not even the same bytes
        for g in (gi, gj, gx):
            if g is not None:
                g.assert_untouched()
    return gi.read(), gj.read(), None if gx is None else gx.read()


def check_against_model(i, j, x, kind, what, expect_sorted=False):
    got = sorted_on_device(i, j, x, kind, expect_sorted)
    CM.assert_equals_model(got, (i, j, x), what)


# ----------------------------------------------------------------------------- device level
@pytest.mark.parametrize("nnz", [0, 1, TP_TILE - 1, TP_TILE, TP_TILE + 1, 3 * TP_TILE + 17])
def test_tile_edges(gpu, nnz):
    rng = np.random.default_rng(nnz)
    i, j = CM.unique_cells(300, 300, nnz, rng)                      # two radix passes on each key
    already = nnz < 2
    check_against_model(i, j, CM.values_for("numeric", nnz, rng), "numeric", f"nnz {nnz}", expect_sorted=already)


@pytest.mark.parametrize("max_i, max_j", list(itertools.product([255, 256, 65536], repeat=2)))
def test_radix_pass_counts(gpu, max_i, max_j):
    """the largest index sizes the passes of its key: 255 -> one, 256 -> two, 65 536 -> three, independently"""
    rng = np.random.default_rng(max_i * 3 + max_j)
    n = 3000
    i = rng.integers(0, max_i + 1, size=n).astype(np.int32)
    j = rng.integers(0, max_j + 1, size=n).astype(np.int32)
    i[17], j[1234] = max_i, max_j
    i[5], j[6] = 0, 0
    check_against_model(i, j, np.arange(n, dtype=np.float64), "numeric", f"maxima {max_i}, {max_j}")


@pytest.mark.parametrize("axis", ["one_row", "one_column"])
def test_degenerate_keys(gpu, axis):
    n = TP_TILE + 300
    rng = np.random.default_rng(5)
    moving = rng.permutation(70000)[:n].astype(np.int32)
    fixed = np.full(n, 41, dtype=np.int32)
    i, j = (fixed, moving) if axis == "one_row" else (moving, fixed)
    check_against_model(i, j, CM.values_for("numeric", n, rng), "numeric", axis)


def test_reverse_sorted_input(gpu):
    n = 2 * TP_TILE + 9
    rng = np.random.default_rng(6)
    i, j = CM.unique_cells(500, 400, n, rng)
    si, sj, sx = CM.model(i, j, CM.values_for("numeric", n, rng))
    check_against_model(si[::-1].copy(), sj[::-1].copy(), sx[::-1].copy(), "numeric", "reversed")


@pytest.mark.parametrize("kind", CM.KINDS)
def test_sorted_input_is_left_alone(gpu, kind):
    n = TP_TILE + 77
    rng = np.random.default_rng(7)
    i, j = CM.repeated_cells(60, 50, n, rng)                        # non-decreasing, with equal neighbours
    si, sj, sx = CM.model(i, j, CM.values_for(kind, n, rng))
    check_against_model(si, sj, sx, kind, "sorted", expect_sorted=True)


def test_entries_of_one_cell_keep_their_input_order(gpu):
    n = TP_TILE + 5
    tags = np.arange(n, dtype=np.float64)
    i, j = np.full(n, 3, dtype=np.int32), np.full(n, 9, dtype=np.int32)
    gi, gj, gx = sorted_on_device(i, j, tags, "numeric", expect_sorted=True)
    assert np.array_equal(gx, tags)
    i[0], j[0] = 4, 0                                               # one entry out of place: the sort runs
    gi, gj, gx = sorted_on_device(i, j, tags, "numeric")
    assert gi.tolist() == [3] * (n - 1) + [4] and gj.tolist() == [9] * (n - 1) + [0]
    assert np.array_equal(gx, np.concatenate([tags[1:], tags[:1]]))


@pytest.mark.parametrize("kind", CM.KINDS)
def test_shuffle_with_repeated_cells(gpu, kind):
    """a tenth of the entries repeat a cell; f64 values carry NaN payloads and -0.0, logicals NA"""
    n = 2 * TP_TILE + 100
    rng = np.random.default_rng(8)
    i, j = CM.unique_cells(700, 300, n, rng)
    rep = n // 10
    i[-rep:], j[-rep:] = i[:rep], j[:rep]
    o = rng.permutation(n)
    x = CM.values_for(kind, n, rng)
    if kind == "numeric":
        assert np.isnan(x).sum() == 2 and (CM.bits(x) == np.uint64(1 << 63)).any()      # rounding makes more -0.0
    if kind == "logical":
        assert (x == CM.NA_LOGICAL).any()
    check_against_model(i[o], j[o], x, kind, f"{kind} with repeats")


@pytest.mark.parametrize("where", ["row", "column", "row_of_sorted"])
def test_negative_index_raises_and_leaves_everything(gpu, where):
    n = TP_TILE + 3
    rng = np.random.default_rng(9)
    i, j = CM.unique_cells(300, 300, n, rng)
    x = rng.normal(size=n)
    if where == "row_of_sorted":                                    # non-decreasing all the same: still an error
        i, j, x = CM.model(i, j, x)
        i[0] = -1
    elif where == "row":
        i[n // 2] = -5
    else:
        j[n - 1] = np.int32(-2147483648)
    rc, _, (gi, gj, gx) = dev_coo_sort(i, j, x, "numeric")
    assert rc != 0 and "negative index" in _lib.load().mx_last_error().decode()
    for g in (gi, gj, gx):
        g.assert_untouched()
    i2, j2, x2 = i.copy(), j.copy(), x.copy()
    with pytest.raises(_lib.MxError, match="negative index"):
        G.sort_coo_indices_numeric(i2, j2, x2)
    assert i2.tobytes() == i.tobytes() and j2.tobytes() == j.tobytes() and x2.tobytes() == x.tobytes()


def test_unsupported_value_kind_is_refused(gpu):
    i, j = np.array([1, 0], np.int32), np.array([0, 0], np.int32)
    gi, gj, gx = GuardedVec(np.int32, data=i), GuardedVec(np.int32, data=j), GuardedVec(np.int32, data=i)
    gws = GuardedVec(np.uint8, n=_lib.load().mxd_coo_sort_workspace_bytes(2))
    was = C.c_int(-1)
    assert _lib.load().mxd_coo_sort(gi.ptr, gj.ptr, gx.ptr, 2, _lib.MX_I32, gws.ptr, C.byref(was), None) != 0
    _sync()
    for g in (gi, gj, gx):
        g.assert_untouched()


# ----------------------------------------------------------------------------- export level
@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: f"{r['kind']}-{r['label']}")
def test_exports_match_the_reference_fixture(gpu, rec):
    inp = (rec["i"], rec["j"], rec["x"])
    got = CM.run(G, rec["kind"], *inp)
    what = f"{rec['kind']} {rec['label']}"
    CM.assert_matches_reference(got, (rec["ri"], rec["rj"], rec["rx"]), what)
    CM.assert_equals_model(got, inp, what)                          # repeated cells: in input order


# ----------------------------------------------------------------------------- device.coo_sort
@pytest.mark.parametrize("byrow", [True, False])
def test_device_coo_sort(gpu, byrow):
    import torch
    from matrixextra_amd import device as D
    n, m, K = TP_TILE + 500, 400, 350
    rng = np.random.default_rng(10)
    i, j = CM.unique_cells(m, K, n, rng)
    x = rng.normal(size=n)
    for values in (x, CM.values_for("logical", n, rng), None):
        di, dj = torch.from_numpy(i).cuda(), torch.from_numpy(j).cuda()
        dx = None if values is None else torch.from_numpy(values).cuda()
        assert D.coo_sort(di, dj, dx, byrow=byrow) is False
        if byrow:
            wi, wj, wx = CM.model(i, j, values)
        else:
            wj, wi, wx = CM.model(j, i, values)
        assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(dj.cpu().numpy(), wj)
        assert dx is None or np.array_equal(CM.bits(dx.cpu().numpy()), CM.bits(wx))
        assert D.coo_sort(di, dj, dx, byrow=byrow) is True          # and now it is sorted
        assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(dj.cpu().numpy(), wj)
    # unique cells: the sorted triplets are the CSR's (the CSC's with byrow=False) entries in storage order
    di, dj, dx = torch.from_numpy(i).cuda(), torch.from_numpy(j).cuda(), torch.from_numpy(x).cuda()
    A = D.coo_to_csr(di, dj, dx, m, K) if byrow else D.coo_to_csr(dj, di, dx, K, m)
    major, minor, vals = D.csr_to_coo(A)
    D.coo_sort(di, dj, dx, byrow=byrow)
    first, second = (di, dj) if byrow else (dj, di)
    assert torch.equal(first, major) and torch.equal(second, minor)
    assert torch.equal(dx.view(torch.int64), vals.view(torch.int64))
    with pytest.raises(ValueError):
        D.coo_sort(di, dj[:-1], dx)


# ----------------------------------------------------------------------------- mirror
@pytest.mark.parametrize("cls, kind", [(mx.dgTMatrix, "numeric"), (mx.lgTMatrix, "logical"), (mx.ngTMatrix, "binary")])
@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("byrow", [True, False])
def test_sort_sparse_indices_of_a_coo(gpu, cls, kind, copy, byrow):
    rng = np.random.default_rng(11)
    n = 500
    i, j = CM.repeated_cells(40, 30, n, rng)
    x = CM.values_for(kind, n, rng)
    T = cls(i.copy(), j.copy(), None if x is None else x.copy(), (40, 30))
    out = mx.sort_sparse_indices(T, copy=copy, byrow=byrow)
    assert (out is not T) if copy else (out is T)
    if byrow:
        wi, wj, wx = CM.model(i, j, x)
    else:
        wj, wi, wx = CM.model(j, i, x)
    assert np.array_equal(out.i, wi) and np.array_equal(out.j, wj)
    assert wx is None or np.array_equal(CM.bits(out.x), CM.bits(wx))
    if copy:
        assert np.array_equal(T.i, i) and np.array_equal(T.j, j) and (x is None or np.array_equal(CM.bits(T.x), CM.bits(x)))
    assert out.Dim == (40, 30)


def test_check_sparse_matrix_sorts_a_coo_under_the_option(gpu, monkeypatch):
    i = np.array([2, 0, 1, 0, 1, 0], np.int32)
    j = np.array([1, 3, 0, 3, 2, 0], np.int32)
    x = np.array([1.5, 2.5, 0.0, 0.5, 4.0, -3.0])
    T = mx.dgTMatrix(i.copy(), j.copy(), x.copy(), (3, 4))
    with pytest.raises(mx.MatrixExtraError, match="not on the accelerated path"):
        mx.check_sparse_matrix(T)
    monkeypatch.setitem(matrices.options, "mxgpu.coo_sort_route", True)
    out = mx.check_sparse_matrix(T)                                 # the zero goes, the rest is sorted
    assert out.i.tolist() == [0, 0, 0, 1, 2] and out.j.tolist() == [0, 3, 3, 2, 1]
    assert out.x.tolist() == [-3.0, 2.5, 0.5, 4.0, 1.5]
    assert np.array_equal(T.i, i) and np.array_equal(T.x, x)
    kept = mx.check_sparse_matrix(T, remove_zeros=False)           # nothing removed: a sorted copy
    assert kept is not T and np.array_equal(T.i, i) and kept.i.tolist() == [0, 0, 0, 1, 1, 2]
    assert kept.x.tolist() == [-3.0, 2.5, 0.5, 0.0, 4.0, 1.5]
