"""NA selectors, `drop` and the CSR scalar lookup of `[` (matrixextra_amd/slice.py), the checks that
need no GPU: with the exports replaced by recorders, the NA fields of get_ij_properties (R/slice.R:111-132), the routine
each selector reaches and the NA lists it hands over, the all-NA branch, the messages, the option gate and the
sparseVector selectors; the numpy model against every golden record; and the new C-ABI entries."""
import ctypes as C

import numpy as np
import pytest

import matrixextra_amd as mx
import na_slice_model as NM
from matrixextra_amd import _lib, exports as G
from matrixextra_amd import slice as S
from matrixextra_amd.assign import assign_csr
from matrixextra_amd.matrices import MatrixExtraError, options

NA = mx.matrices.NA_INTEGER
NA_LGL = mx.matrices.NA_LOGICAL
RECORDS, META = NM.load()


def _seq(a, rev=False):
    a = np.asarray(a, dtype=np.int64)
    return a.size < 2 or bool(np.all(np.diff(a) == (-1 if rev else 1)))


@pytest.fixture
def calls(monkeypatch):
    """Replaces the device-backed exports with recorders; returns the list of (name, args)."""
    log = []
    monkeypatch.setattr(G, "check_is_seq", lambda a: _seq(a))
    monkeypatch.setattr(G, "check_is_rev_seq", lambda a: _seq(a, rev=True))
    monkeypatch.setattr(G, "rows_are_sorted", lambda p, j: True)
    monkeypatch.setattr(G, "csr_to_coo", lambda p: np.repeat(np.arange(p.size - 1, dtype=np.int32), np.diff(p)))

    def rec(name, result):
        def f(*args, **kw):
            log.append((name, args))
            return result(*args, **kw) if callable(result) else result
        monkeypatch.setattr(G, name, f)

    def csr(n_rows):
        return dict(indptr=np.zeros(n_rows + 1, np.int32), indices=np.zeros(0, np.int32), values=np.zeros(0))

    for k in ("numeric", "logical", "binary"):
        rec("copy_csr_rows_" + k, lambda *a: csr(a[-1].size))
        rec("copy_csr_arbitrary_" + k, lambda *a: csr(a[-2].size))
        rec("copy_csr_rows_col_seq_" + k, lambda *a: csr(a[-3].size))
        rec("slice_coo_arbitrary_" + k, lambda *a, k=k: dict(
            ii=np.zeros(0, np.int32), jj=np.zeros(0, np.int32),
            xx=None if k == "binary" else np.zeros(0, np.float64 if k == "numeric" else np.int32)))
    for name in ("set_single_row_to_const", "set_arbitrary_rows_to_const", "set_rowseq_to_const",
                 "set_single_col_to_const", "set_arbitrary_cols_to_const", "set_colseq_to_const"):
        rec(name, lambda p, j, x, *a: dict(indptr=p, indices=j, values=x))
    for k in ("numeric", "logical"):
        rec("inject_NAs_inplace_coo_" + k, dict(ii=np.zeros(0, np.int32), jj=np.zeros(0, np.int32), xx=np.zeros(0)))
    rec("extract_single_val_csr_numeric", 2.5)
    rec("extract_single_val_csr_logical", int(NA_LGL))
    rec("extract_single_val_csr_binary", 0.0)
    rec("slice_coo_single_numeric", 2.5)
    rec("repeat_indices_n_times", lambda ix, rem, L, n: NM.repeat_indices(ix, rem, L, n))
    rec("entries_to_dense_vector", lambda pos, vals, n, logical=False: np.zeros(n))
    rec("coo_to_csr", lambda i, j, x, m, n: csr(m))
    rec("sort_vector_indices_binary", None)
    rec("sort_vector_indices_logical", None)
    return log


def _names(log):
    return [c[0] for c in log]


def _R(cls=mx.dgRMatrix, names=False):
    p = np.array([0, 2, 2, 3, 5, 5], np.int32)
    j = np.array([1, 3, 2, 0, 3], np.int32)
    x = None if cls is mx.ngRMatrix else (np.array([1.0, 2.0, 3.0, 4.0, 5.0]) if cls is mx.dgRMatrix
                                          else np.array([1, 0, 1, 1, NA_LGL], np.int32))
    return cls(p, j, x, (5, 4), [["a", "b", "c", "d", "e"], ["w", "x", "y", "z"]] if names else None)


def _T(cls=mx.dgTMatrix, names=False):
    i = np.array([0, 3, 2, 4, 0], np.int32)
    j = np.array([1, 0, 2, 3, 1], np.int32)
    x = None if cls is mx.ngTMatrix else (np.array([1.0, 2.0, 3.0, 4.0, 5.0]) if cls is mx.dgTMatrix
                                          else np.array([1, 0, 1, 1, NA_LGL], np.int32))
    return cls(i, j, x, (5, 4), [["a", "b", "c", "d", "e"], ["w", "x", "y", "z"]] if names else None)


@pytest.fixture
def drop_route():
    options["mxgpu.slice_drop_route"] = True
    yield
    options.pop("mxgpu.slice_drop_route", None)
    options["MatrixExtra.drop_sparse"] = False


# ---- get_indices_integer / get_ij_properties ------------------------------------------------------------------------
@pytest.mark.parametrize("sel", [np.array([2, NA, 4, NA], np.int32), np.array([2.0, np.nan, 4.7, np.nan]),
                                 np.array([2, None, 4, None], dtype=object), [2, None, 4.0, float("nan")]])
def test_the_three_spellings_of_NA_read_alike(sel):
    assert list(S.get_indices_integer(sel, 5, None)) == [2, NA, 4, NA]


def test_NA_is_exempt_from_the_bounds_check_and_the_exclusion_rule():
    assert list(S.get_indices_integer(np.array([NA, 5], np.int32), 5, None)) == [NA, 5]
    with pytest.raises(MatrixExtraError, match="not present in matrix"):
        S.get_indices_integer(np.array([1, NA, 6], np.int32), 5, None)
    with pytest.raises(MatrixExtraError, match="can't mix NAs with negative subscripts"):
        S.get_indices_integer(np.array([-1.0, np.nan]), 5, None)
    with pytest.raises(MatrixExtraError, match="can't mix positive and negative"):
        S.get_indices_integer(np.array([-1, 2, NA], np.int32), 5, None)
    assert list(S.get_indices_integer(np.array(["c", None, "a"], dtype=object), 5, list("abcde"))) == [3, NA, 1]
    assert list(S.get_indices_integer([-1, -5], 5, None)) == [2, 3, 4]                    # as before


def test_NA_fields_of_get_ij_properties(calls):
    P = S.get_ij_properties(_R(names=True), np.array([NA, 4, 5, NA], np.int32), np.array([2.0, np.nan]))
    assert (P.i_has_NA, P.i_all_NA, P.j_has_NA, P.j_all_NA) == (True, False, True, False)
    assert list(P.i) == [4, 4, 5, 4] and list(P.i_NAs) == [1, 4] and P.i.dtype == np.int32
    assert list(P.j) == [2, 2] and list(P.j_NAs) == [2]
    assert not (P.all_i or P.all_j or P.i_is_seq or P.j_is_seq or P.i_is_rev_seq or P.j_is_rev_seq)
    assert (P.n_row, P.n_col) == (4, 2) and P.row_names == ["d", "d", "e", "d"] and P.col_names == ["x", "x"]
    assert calls == []                                  # the flag checks are skipped for an axis with NAs
    P = S.get_ij_properties(_R(names=True), [None, None], None)
    assert (P.i_has_NA, P.i_all_NA, P.i_NAs) == (True, True, None) and list(P.i) == [NA, NA]
    assert P.row_names is None and P.all_j and not P.j_has_NA and P.j_NAs is None
    P = S.get_ij_properties(_R(), [2, 3], None)
    assert (P.i_has_NA, P.i_all_NA, P.i_NAs, P.j_has_NA) == (False, False, None, False) and P.i_is_seq
    assert S.find_first_non_na(np.array([NA, NA, 7, 2], np.int32)) == 7
    assert S.find_first_non_na(np.array([NA], np.int32)) == NA and S.find_first_non_na(np.zeros(0, np.int32)) == NA


# ---- which routine a selector reaches -------------------------------------------------------------------------------
@pytest.mark.parametrize("cls, kind", [(mx.dgRMatrix, "numeric"), (mx.lgRMatrix, "logical"), (mx.ngRMatrix, "binary")])
def test_csr_rows_with_an_NA_are_gathered_then_assigned_NA(calls, cls, kind):
    out = S.subset_csr(_R(cls, names=True), np.array([1, NA, 3], np.int32))
    assert _names(calls) == ["copy_csr_rows_" + kind, "set_single_row_to_const"]
    assert list(calls[0][1][-1]) == [0, 0, 2]                              # the NA replaced by the first index
    p, j, x, ncol, row, value = calls[1][1]
    assert (ncol, row) == (4, 1) and np.isnan(value) and np.array([value]).view(np.uint64)[0] == NM.NA_REAL_BITS
    assert x.dtype == np.float64                                            # the assignment runs on a dgRMatrix
    assert type(out) is (mx.dgRMatrix if cls is mx.dgRMatrix else mx.lgRMatrix)
    assert out.Dim == (3, 4) and out.Dimnames == [["a", None, "c"], ["w", "x", "y", "z"]]


def test_csr_NA_rows_and_columns_take_two_assignments(calls):
    out = S.subset_csr(_R(names=True), np.array([NA, 2, NA, 5], np.int32), np.array([4.0, np.nan, 1.0]))
    assert _names(calls) == ["copy_csr_arbitrary_numeric", "set_arbitrary_rows_to_const", "set_single_col_to_const"]
    assert list(calls[0][1][-2]) == [1, 1, 1, 4] and list(calls[0][1][-1]) == [3, 3, 0]
    assert list(calls[1][1][3]) == [0, 2] and calls[1][1][4] == 3 and np.isnan(calls[1][1][5])
    assert calls[2][1][3:5] == (3, 1) and np.isnan(calls[2][1][5])
    assert out.Dim == (4, 3) and out.Dimnames == [[None, "b", None, "e"], ["z", None, "w"]]


@pytest.mark.parametrize("cls, kind, out_cls", [(mx.dgTMatrix, "numeric", mx.dgTMatrix),
                                                (mx.lgTMatrix, "logical", mx.lgTMatrix),
                                                (mx.ngTMatrix, "logical", mx.lgTMatrix)])
def test_coo_selectors_with_NA_reach_the_injection_with_both_lists(calls, cls, kind, out_cls):
    out = S.subset_coo(_T(cls, names=True), np.array([1, NA, 3, NA], np.int32), np.array([NA, 2], np.int32))
    assert _names(calls)[-1] == "inject_NAs_inplace_coo_" + kind and len(calls) == 2
    assert calls[0][0].startswith("slice_coo_arbitrary_")
    ii, jj, xx, rows_na, cols_na, nrows, ncols = calls[1][1]
    assert list(rows_na) == [1, 3] and list(cols_na) == [0] and (nrows, ncols) == (4, 2)
    assert rows_na.dtype == np.int32 and xx.dtype == (np.float64 if kind == "numeric" else np.int32)
    assert type(out) is out_cls and out.Dim == (4, 2) and out.Dimnames == [["a", None, "c", None], [None, "x"]]
    calls.clear()
    S.subset_coo(_T(cls), np.array([2, 1]), np.array([1.0, np.nan, 3.0]))
    assert list(calls[1][1][3]) == [] and list(calls[1][1][4]) == [1] and calls[1][1][3].dtype == np.int32


def test_selectors_without_NA_reach_no_injection(calls):
    S.subset_coo(_T(), np.array([3, 1]), np.array([2, 4]))
    S.subset_csr(_R(), np.array([3, 1]), np.array([2, 4]))
    assert _names(calls) == ["slice_coo_arbitrary_numeric", "copy_csr_arbitrary_numeric"]


@pytest.mark.parametrize("make, cls, want", [(_R, mx.dgRMatrix, mx.dgRMatrix), (_R, mx.ngRMatrix, mx.lgRMatrix),
                                             (_T, mx.dgTMatrix, mx.dgTMatrix), (_T, mx.lgTMatrix, mx.lgTMatrix)])
def test_an_axis_that_is_all_NA_needs_no_device(calls, make, cls, want):
    sub = S.subset_csr if make is _R else S.subset_coo
    out = sub(make(cls, names=True), [None, None, None], np.array([2, 1]))
    assert calls == [] and type(out) is want and out.Dim == (3, 2) and out.Dimnames == [None, ["x", "w"]]
    assert np.isnan(out.toarray()).all()
    if want in (mx.lgRMatrix, mx.lgTMatrix):
        assert out.x.dtype == np.int32 and (out.x == NA_LGL).all()
    else:
        assert (out.x.view(np.uint64) == NM.NA_REAL_BITS).all()
    out = sub(make(cls, names=True), np.array([np.nan]), None)
    assert out.Dim == (1, 4) and np.isnan(out.toarray()).all() and out.Dimnames == [None, ["w", "x", "y", "z"]]
    out = sub(make(cls), np.array([2, NA], np.int32), [None])
    assert calls == [] and out.Dim == (2, 1) and np.isnan(out.toarray()).all()


def test_assignment_still_refuses_NA_indices(calls):
    with pytest.raises(MatrixExtraError, match="Indices contain NAs."):
        assign_csr(_R(), np.array([1, NA], np.int32), None, 1.0)
    with pytest.raises(MatrixExtraError, match="Indices contain NAs."):
        assign_csr(_R(), None, np.array([np.nan, 2.0]), 1.0)


def test_an_NA_scalar_of_a_coo_is_NA_real(calls):
    for i, j in ((np.nan, 2), (2, float("nan")), (int(NA), 1)):
        got = S.subset_coo(_T(), i, j)
        assert np.array([got]).view(np.uint64)[0] == NM.NA_REAL_BITS
    one = S.subset_coo(_T(mx.lgTMatrix), float("nan"), 2, drop=False)
    assert type(one) is mx.lgTMatrix and one.Dim == (1, 1) and list(one.x) == [NA_LGL] and calls == []
    assert S.subset_coo(_T(), 1, 2) == 2.5 and _names(calls) == ["slice_coo_single_numeric"]


# ---- the option gate: drop and the CSR scalar lookup -----------------------------------------------------------------
def test_with_the_option_off_nothing_drops_and_scalars_take_the_vector_route(calls):
    assert "mxgpu.slice_drop_route" not in options
    out = S.subset_csr(_R(), 2, 3, drop=True)
    assert type(out) is mx.dgRMatrix and out.Dim == (1, 1) and _names(calls) == ["copy_csr_rows_col_seq_numeric"]
    out = S.subset_csr(_R(), np.array([4]), None, drop=True)
    assert type(out) is mx.dgRMatrix and out.Dim == (1, 4)
    out = S.subset_coo(_T(), np.array([4, 2]), np.array([2]), drop=True)
    assert type(out) is mx.dgTMatrix and out.Dim == (2, 1)
    T = _T()
    assert S.subset_coo(T, None, None, drop=True) is T
    assert "entries_to_dense_vector" not in _names(calls) and "extract_single_val_csr_numeric" not in _names(calls)


def test_the_csr_scalar_route(calls, drop_route):
    assert S.subset_csr(_R(), 2, 3.9, drop=True) == 2.5
    assert calls[-1][0] == "extract_single_val_csr_numeric" and calls[-1][1][3:] == (1, 2)
    assert S.subset_csr(_R(mx.lgRMatrix), 1, 1, drop=True) == NA_LGL
    assert S.subset_csr(_R(mx.ngRMatrix), [1], [1], drop=True) == 0.0
    one = S.subset_csr(_R(names=True), 4, 1, drop=False)
    assert type(one) is mx.dgRMatrix and one.Dim == (1, 1) and list(one.p) == [0, 1] and list(one.x) == [2.5]
    assert one.Dimnames == [["d"], ["w"]]
    empty = S.subset_csr(_R(mx.ngRMatrix), 4, 1, drop=False)
    assert type(empty) is mx.ngRMatrix and list(empty.p) == [0, 0] and empty.j.size == 0
    n = len(calls)
    got = S.subset_csr(_R(), np.nan, 2, drop=True)
    assert np.array([got]).view(np.uint64)[0] == NM.NA_REAL_BITS and len(calls) == n
    with pytest.raises(MatrixExtraError, match="Subscript out of bounds."):
        S.subset_csr(_R(), 6, 1)
    with pytest.raises(MatrixExtraError, match="Subscript out of bounds."):
        S.subset_csr(_R(), 1, 5)
    assert S.subset_csr(_R(), 0, 1, drop=True) == 0.0 and len(calls) == n


def test_drop_gives_a_vector_and_python_keys_never_drop(calls, drop_route):
    v = S.subset_csr(_R(), np.array([4]), None, drop=True)
    assert isinstance(v, np.ndarray) and v.shape == (4,) and calls[-1][0] == "entries_to_dense_vector"
    assert calls[-1][1][2] == 4
    v = S.subset_coo(_T(), np.array([4, 2]), np.array([2]))                        # drop defaults to TRUE there
    assert isinstance(v, np.ndarray) and v.shape == (2,)
    m = S.subset_csr(_R(), np.array([4]), None, drop=False)
    assert type(m) is mx.dgRMatrix and m.Dim == (1, 4)
    m = S.subset_csr(_R(), np.array([4, 1]), None, drop=True)
    assert type(m) is mx.dgRMatrix and m.Dim == (2, 4)
    assert type(_R()[3]) is mx.dgRMatrix and _R()[3].Dim == (1, 4)                # `[` in Python style
    assert type(_T()[[3, 1], 2]) is mx.dgTMatrix and type(_R()[3, 1]) is mx.dgRMatrix
    options["MatrixExtra.drop_sparse"] = True
    n = len(calls)
    v = S.subset_csr(_R(), np.array([4]), None, drop=True)
    assert type(v) is mx.matrices.dsparseVector and v.length == 4 and len(calls) == n   # no dense vector is made


# ---- sparseVector selectors -----------------------------------------------------------------------------------------
def test_sparse_vector_selectors(calls):
    n = mx.matrices.nsparseVector([1, 4, 5], None, 5)
    assert list(S.get_indices_integer(n, 5, None)) == [1, 4, 5] and "repeat_indices_n_times" not in _names(calls)
    short = mx.matrices.nsparseVector([1, 3], None, 3)
    assert list(S.get_indices_integer(short, 8, None)) == [1, 3, 4, 6, 7]       # recycled: 1 3 | 4 6 | 7
    ix, rem, L, want = [c for c in calls if c[0] == "repeat_indices_n_times"][-1][1]
    assert list(ix) == [1, 3] and list(rem) == [1] and (L, want) == (3, 8)
    assert list(S.get_indices_integer(short, 6, None)) == [1, 3, 4, 6]
    assert list([c for c in calls if c[0] == "repeat_indices_n_times"][-1][1][1]) == []
    lv = mx.matrices.lsparseVector([1, 2, 4], [1, 0, 1], 4)
    assert list(S.get_indices_integer(lv, 4, None)) == [1, 4]                    # a stored FALSE selects nothing
    lna = mx.matrices.lsparseVector([1, 2], [NA_LGL, 1], 3)
    assert list(S.get_indices_integer(lna, 5, None)) == [NA, 2, NA, 5]          # NA T F | NA T
    with pytest.raises(MatrixExtraError, match="Dimension of indexing vector is larger than matrix to subset."):
        S.get_indices_integer(mx.matrices.nsparseVector([1], None, 6), 5, None)
    calls.clear()
    S.subset_csr(_R(), short, None)
    assert calls[-1][0] == "copy_csr_rows_numeric" and list(calls[-1][1][-1]) == [0, 2, 3]


# ---- the model against the reference's records, and the ABI ------------------------------------------------------------
def test_the_model_matches_every_golden_record():
    assert len(RECORDS) >= 300 and META["flags"]
    for r in RECORDS:
        got = NM.model_of(r)
        A = r["arrays"]
        if r["name"].startswith("inject"):
            want = (A["out_ii"], A["out_jj"], A["out_xx"] if r["name"].endswith("logical") else A["out_xx_f64"])
            for g, w in zip(got, want):
                assert g.dtype == w.dtype, (r["name"], r["label"])
                same = np.array_equal(NM.bits(g), NM.bits(w)) if g.dtype == np.float64 else np.array_equal(g, w)
                assert same, (r["name"], r["label"])
        elif r["name"].startswith("extract"):
            assert got == r["result_bits"], (r["name"], r["label"])
        else:
            assert np.array_equal(got, A["out"]), r["label"]


def test_the_remainder_lines_are_the_swap_loops():
    assert list(NM.remainder_lines(4, [0, 3])) == [2, 1]                         # not ascending
    assert list(NM.remainder_lines(5, [])) == [0, 1, 2, 3, 4] and list(NM.remainder_lines(3, [0, 1, 2])) == []
    assert list(NM.remainder_lines(10, [4, 5, 6, 7, 8])) == [0, 1, 2, 3, 9]


def test_the_new_entries_are_bound_from_the_header():
    protos = _lib.HEADER.functions
    i32p, vp = C.c_void_p, C.c_void_p
    assert protos["mxd_coo_inject_na_count"] == (C.c_int, (C.c_int, C.c_int, i32p, i32p, C.c_int64, i32p, C.c_int64,
                                                          i32p, C.c_int64, vp, i32p, vp, vp))
    assert len(protos["mxd_coo_inject_na_fill"][1]) == 17
    # no size function of its own: the kept pass takes compact's workspace, whose sizes are on record
    assert not [n for n in protos if "inject_na" in n and n.endswith("_workspace_bytes")]
    assert protos["mxd_csr_single"][1][:2] == (C.c_int, i32p) and len(protos["mxd_csr_single"][1]) == 12
    assert protos["mxd_repeat_indices"] == (C.c_int, (i32p, C.c_int64, i32p, C.c_int64, C.c_int, C.c_int, i32p, vp))
    assert len(protos["mxd_entries_to_dense_vector"][1]) == 8
    assert len(protos["mx_inject_NAs_inplace_coo_begin"][1]) == 13
    assert len(protos["mx_extract_single_val_csr"][1]) == 9 and len(protos["mx_repeat_indices_n_times"][1]) == 7
    lib = _lib.load()
    for name in ("mxd_coo_inject_na_count", "mxd_coo_inject_na_fill", "mxd_csr_single", "mxd_repeat_indices",
                 "mxd_entries_to_dense_vector", "mx_inject_NAs_inplace_coo_begin", "mx_extract_single_val_csr",
                 "mx_repeat_indices_n_times", "mx_entries_to_dense_vector"):
        assert tuple(getattr(lib, name).argtypes) == protos[name][1]
    assert lib.mx_abi_version() == 1 == _lib.MXGPU_ABI_VERSION


def test_exports_carry_the_reference_signatures():
    import inspect
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_signatures.json")) as f:
        sigs = json.load(f)
    for name in ("inject_NAs_inplace_coo_numeric", "inject_NAs_inplace_coo_logical", "extract_single_val_csr_numeric",
                 "extract_single_val_csr_logical", "extract_single_val_csr_binary", "repeat_indices_n_times"):
        assert len(inspect.signature(getattr(G, name)).parameters) == sigs[name]["arity"], name
    assert list(inspect.signature(G.inject_NAs_inplace_coo_numeric).parameters) == [
        "ii", "jj", "xx", "rows_na_", "cols_na_", "nrows", "ncols"]


def test_argument_checks_of_the_exports_need_no_device():
    lib = _lib.load()
    res, info = C.c_void_p(), _lib.ResultInfo()
    x = np.zeros(1)
    i = np.zeros(1, np.int32)
    assert lib.mx_inject_NAs_inplace_coo_begin(_lib.ptr(i), _lib.ptr(i), _lib.ptr(x), _lib.MX_NONE, 1, None, 0, None, 0,
                                               1, 1, C.byref(res), C.byref(info)) != 0
    assert "unsupported value dtype" in lib.mx_last_error().decode()
    found = C.c_int(7)
    p = np.array([0, 0, 0], np.int32)
    assert lib.mx_extract_single_val_csr(_lib.ptr(p), 2, None, None, _lib.MX_F64, 1, 0, C.byref(found), None) == 0
    assert found.value == 0                                                      # an empty row: no device call
    assert lib.mx_extract_single_val_csr(_lib.ptr(p), 2, None, None, _lib.MX_F64, 2, 0, C.byref(found), None) != 0
    assert "row index 2 outside [0, 2)" in lib.mx_last_error().decode()
    assert lib.mx_repeat_indices_n_times(None, 0, None, 0, 0, 5, None) != 0
    assert "not positive" in lib.mx_last_error().decode()
    with pytest.raises(ValueError):
        G.repeat_indices_n_times([1], [], 0, 3)
    assert G.inject_NAs_inplace_coo_numeric([0], [0], [1.0], [], [], 1, 1) == {}
