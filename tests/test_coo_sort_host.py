"""The COO sort's host layers, checked without a GPU: the C-ABI entries are declared and exported, the Python exports
check their arguments before any device call, and the mirror (sort_sparse_indices of a TsparseMatrix,
check_sparse_matrix under options["mxgpu.coo_sort_route"]) routes, copies and orders as R/utils.R:85-124 and :439-489
do, with the three exports replaced by the numpy model of tests/coo_sort_model.py."""
import os
import re

import numpy as np
import pytest

import coo_sort_model as CM
import matrixextra_amd as mx
from matrixextra_amd import _lib, exports, matrices

CLASSES = {mx.dgTMatrix: "numeric", mx.lgTMatrix: "logical", mx.ngTMatrix: "binary"}


def _coo(cls=mx.dgTMatrix):
    """(2,1) (0,3) (1,0) (0,3) (1,2) (0,0): unsorted in both orders, one repeated cell, no zero value"""
    i = np.array([2, 0, 1, 0, 1, 0], np.int32)
    j = np.array([1, 3, 0, 3, 2, 0], np.int32)
    x = {mx.dgTMatrix: np.array([1.5, 2.5, -1.0, 0.5, 4.0, -3.0]), mx.lgTMatrix: np.array([1, 1, 1, CM.NA_LOGICAL, 1, 1], np.int32),
         mx.ngTMatrix: None}[cls]
    return cls(i, j, x, (3, 4), [["a", "b", "c"], None])


@pytest.fixture
def modelled(monkeypatch):
    """The three exports replaced by the model, in place like the real ones; the calls are recorded."""
    calls = []

    def make(kind):
        def f(indices1, indices2, values=None):
            assert (values is None) == (kind == "binary")
            calls.append((kind, indices1, indices2, values))
            si, sj, sx = CM.model(indices1, indices2, values)
            indices1[...], indices2[...] = si, sj
            if values is not None:
                values[...] = sx
        return f
    for kind in CM.KINDS:
        monkeypatch.setattr(exports, "sort_coo_indices_" + kind, make(kind))
    return calls


def test_entry_points_declared_and_exported():
    wanted = {"mx_sort_coo_indices", "mxd_coo_sort", "mxd_coo_sort_workspace_bytes"}
    assert wanted <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in wanted)
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    proto = re.search(r"/\*(?:(?!\*/).)*\*/\s*int mx_sort_coo_indices\(int32_t \*ii, int32_t \*jj, void \*xx, int64_t nnz, "
                      r"int value_dtype\);", header, flags=re.S)
    assert proto and "src/misc.cpp:387-457" in proto.group(0)
    for kind in CM.KINDS:
        assert callable(getattr(exports, "sort_coo_indices_" + kind))
    assert 0 < lib.mxd_coo_sort_workspace_bytes(1000) < lib.mxd_coo_sort_workspace_bytes(1 << 24)
    assert _lib.load().mx_abi_version() == _lib.MXGPU_ABI_VERSION == 1            # entries were added, none changed


def test_more_entries_than_int32_are_refused_before_anything_is_allocated():
    """both levels look at the count first: no pointer is read and no device is needed to be told so"""
    import ctypes as C
    lib = _lib.load()
    was = C.c_int(-1)
    assert lib.mxd_coo_sort(None, None, None, 2**31, _lib.MX_NONE, None, C.byref(was), None) != 0
    assert "exceed R's int32 index range" in lib.mx_last_error().decode()
    assert lib.mx_sort_coo_indices(None, None, None, 2**31, _lib.MX_NONE) != 0
    assert "exceed R's int32 index range" in lib.mx_last_error().decode()
    assert lib.mx_sort_coo_indices(None, None, None, -1, _lib.MX_NONE) != 0
    assert lib.mx_sort_coo_indices(None, None, None, 0, _lib.MX_F64) == 0          # nothing to sort


def test_shim_and_overlay_carry_the_three_routines():
    import rshim_registry
    for name, nargs in (("sort_coo_indices_numeric", 3), ("sort_coo_indices_logical", 3), ("sort_coo_indices_binary", 2)):
        rshim_registry.assert_shim_and_overlay_carry(name, nargs)


def test_exports_check_their_arguments_before_any_device_call():
    i, j, x = np.array([1, 0], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0])
    with pytest.raises(TypeError, match="indices1 must be a contiguous int32"):
        exports.sort_coo_indices_numeric(i.astype(np.int64), j, x)
    with pytest.raises(TypeError, match="indices2 must be a contiguous int32"):
        exports.sort_coo_indices_binary(i, np.array([0, 9, 1, 9], np.int32)[::2])
    with pytest.raises(TypeError, match="indices1 must be a contiguous int32"):
        exports.sort_coo_indices_binary([1, 0], j)
    with pytest.raises(TypeError, match="values must be a contiguous float64"):
        exports.sort_coo_indices_numeric(i, j, x.astype(np.float32))
    with pytest.raises(TypeError, match="values must be a contiguous int32"):
        exports.sort_coo_indices_logical(i, j, x)
    with pytest.raises(ValueError, match="indices1 and indices2 have different lengths"):
        exports.sort_coo_indices_binary(i, j[:1])
    with pytest.raises(ValueError, match="indices1 and values have different lengths"):
        exports.sort_coo_indices_numeric(i, j, x[:1])
    assert (i.tolist(), j.tolist(), x.tolist()) == ([1, 0], [0, 1], [1.0, 2.0])


@pytest.mark.parametrize("cls", list(CLASSES))
def test_sorts_in_place_and_returns_the_same_object(modelled, cls):
    T = _coo(cls)
    i, j, x = T.i, T.j, T.x
    want = CM.model(i.copy(), j.copy(), None if x is None else x.copy())
    out = mx.sort_sparse_indices(T)
    assert out is T and T.i is i and T.j is j and T.x is x
    assert np.array_equal(i, want[0]) and np.array_equal(j, want[1]) and (x is None or np.array_equal(x, want[2]))
    assert i.tolist() == [0, 0, 0, 1, 1, 2] and j.tolist() == [0, 3, 3, 0, 2, 1]
    if cls is mx.dgTMatrix:
        assert x.tolist() == [-3.0, 2.5, 0.5, -1.0, 4.0, 1.5]                    # the repeated (0,3) in input order
    assert [c[0] for c in modelled] == [CLASSES[cls]] and modelled[0][1] is i and modelled[0][2] is j
    assert T.Dim == (3, 4) and T.Dimnames == [["a", "b", "c"], None]


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("byrow", [True, False])
def test_copy_leaves_the_input_alone_and_shares_nothing(modelled, cls, byrow):
    T = _coo(cls)
    before = (T.i.copy(), T.j.copy(), None if T.x is None else T.x.copy())
    out = mx.sort_sparse_indices(T, copy=True, byrow=byrow)
    assert out is not T and type(out) is cls and out.Dim == T.Dim and out.Dimnames == T.Dimnames
    assert T.i.tobytes() == before[0].tobytes() and T.j.tobytes() == before[1].tobytes()
    assert T.x is None or T.x.tobytes() == before[2].tobytes()
    for a in (out.i, out.j, out.x):
        for b in (T.i, T.j, T.x):
            assert a is None or b is None or not np.shares_memory(a, b)
    if byrow:
        want = CM.model(*before)
    else:
        sj, si, sx = CM.model(before[1], before[0], before[2])
        want = (si, sj, sx)
    assert np.array_equal(out.i, want[0]) and np.array_equal(out.j, want[1])
    assert out.x is None or np.array_equal(out.x, want[2])


def test_byrow_false_sorts_by_column_then_row(modelled):
    T = _coo()
    out = mx.sort_sparse_indices(T, byrow=False)
    assert out is T
    assert T.j.tolist() == [0, 0, 1, 2, 3, 3] and T.i.tolist() == [0, 1, 2, 1, 0, 0]
    assert T.x.tolist() == [-3.0, -1.0, 1.5, 4.0, 2.5, 0.5]
    assert modelled[0][1] is T.j and modelled[0][2] is T.i                      # the export sees (j, i)
    # the same as sorting the t_shallow of T by row and turning it back (R/utils.R:89-90, :123-124)
    U = mx.t_shallow(mx.sort_sparse_indices(mx.t_shallow(_coo())))
    assert np.array_equal(U.i, T.i) and np.array_equal(U.j, T.j) and np.array_equal(U.x, T.x) and U.Dim == T.Dim


def test_check_valid_matrix_speaks_before_any_export(modelled):
    T = _coo()
    T.j = T.j[:-1]
    with pytest.raises(mx.MatrixExtraError, match="row and column indices have different length"):
        mx.sort_sparse_indices(T)
    T = _coo()
    T.x = T.x[:-1]
    with pytest.raises(mx.MatrixExtraError, match="values and indices have different number of entries"):
        mx.sort_sparse_indices(T, copy=True)
    T = _coo()
    T.Dim = (-1, 4)
    with pytest.raises(mx.MatrixExtraError, match="invalid number of rows"):
        mx.sort_sparse_indices(T, byrow=False)
    assert modelled == []


def test_other_layouts_take_byrow_and_stay_as_they_were(monkeypatch):
    seen = []
    monkeypatch.setattr(exports, "sort_sparse_indices_inplace", lambda p, j, x=None: seen.append((p, j, x)))
    X = mx.dgRMatrix(np.array([0, 2, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 2.0]), (2, 2))
    for byrow in (True, False):
        assert mx.sort_sparse_indices(X, byrow=byrow) is X
    assert len(seen) == 2 and all(s[1] is X.j for s in seen)


# ----------------------------------------------------------------------------- check_sparse_matrix
@pytest.fixture
def cleanup_on_host(monkeypatch):
    """check_valid_coo_matrix and remove_zero_valued_coo_* as numpy restatements (no device here)"""
    monkeypatch.setattr(exports, "check_valid_coo_matrix", lambda ii, jj, nrows, ncols: None)

    def remove(ii, jj, xx, na_rm):
        keep = xx != 0
        if keep.all():
            return {"ii": ii, "jj": jj, "xx": xx}
        return {"ii": ii[keep].copy(), "jj": jj[keep].copy(), "xx": xx[keep].copy()}
    monkeypatch.setattr(exports, "remove_zero_valued_coo_numeric", remove)
    monkeypatch.setattr(exports, "remove_zero_valued_coo_logical", remove)


@pytest.mark.parametrize("cls", list(CLASSES))
def test_check_sparse_matrix_refuses_a_coo_with_the_option_off(modelled, cls):
    assert not matrices.options.get("mxgpu.coo_sort_route", False)
    with pytest.raises(mx.MatrixExtraError, match=re.escape(
            "Sorting the indices of a TsparseMatrix (sort_coo_indices_*, R/utils.R:22-161) is not on the accelerated "
            "path; call check_sparse_matrix(X, sort=False).")):
        mx.check_sparse_matrix(_coo(cls))
    assert modelled == []


@pytest.mark.parametrize("cls", list(CLASSES))
def test_check_sparse_matrix_sorts_a_copy_when_nothing_was_removed(modelled, cleanup_on_host, monkeypatch, cls):
    monkeypatch.setitem(matrices.options, "mxgpu.coo_sort_route", True)
    T = _coo(cls)
    before = (T.i.copy(), T.j.copy(), None if T.x is None else T.x.copy())
    out = mx.check_sparse_matrix(T)
    assert out is not T and type(out) is cls                                   # copy = (nnz_before == nnz_after)
    assert T.i.tobytes() == before[0].tobytes() and T.j.tobytes() == before[1].tobytes()
    assert not np.shares_memory(out.i, T.i) and not np.shares_memory(out.j, T.j)
    want = CM.model(*before)
    assert np.array_equal(out.i, want[0]) and np.array_equal(out.j, want[1])
    assert out.x is None or np.array_equal(out.x, want[2])
    assert [c[0] for c in modelled] == [CLASSES[cls]]


def test_check_sparse_matrix_sorts_in_place_what_the_removal_made(modelled, cleanup_on_host, monkeypatch):
    monkeypatch.setitem(matrices.options, "mxgpu.coo_sort_route", True)
    T = _coo()
    T.x[2] = 0.0                                                               # (1,0) goes
    kept = np.array([0, 1, 3, 4, 5])
    before = (T.i.copy(), T.j.copy(), T.x.copy())
    out = mx.check_sparse_matrix(T)
    assert T.i.tobytes() == before[0].tobytes() and T.x.tobytes() == before[2].tobytes()   # the removal made new arrays
    want = CM.model(before[0][kept], before[1][kept], before[2][kept])
    assert np.array_equal(out.i, want[0]) and np.array_equal(out.j, want[1]) and np.array_equal(out.x, want[2])
    assert len(modelled) == 1 and modelled[0][1] is out.i                      # copy=False: sorted where they are
    # sort=False never reaches the sort, option or not
    assert mx.check_sparse_matrix(_coo(), sort=False).i.tolist() == _coo().i.tolist() and len(modelled) == 1
