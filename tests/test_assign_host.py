"""Host logic of `[<-` for a dgRMatrix (matrixextra_amd/assign.py, R/assignment.R:37-513), with the native routines
stubbed: which set_* export each selector shape reaches and with which arguments, every message and refusal, the
all / all cases that never reach native code, and the R-side shim and overlay carrying the same twenty-two names."""
import os
import re
import warnings

import numpy as np
import pytest

import assign_model as AM
import matrixextra_amd as mx
from matrixextra_amd import assign as A
from matrixextra_amd import exports as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = mx.NA_REAL


def _seq(a, rev=False):
    a = np.asarray(a, dtype=np.int64)
    return bool(np.all(np.diff(a) == (-1 if rev else 1)))


@pytest.fixture
def calls(monkeypatch):
    """Every set_* export (and the row gather) replaced by a recorder that returns its inputs."""
    seen = []
    monkeypatch.setattr(G, "check_is_seq", lambda a: _seq(a))
    monkeypatch.setattr(G, "check_is_rev_seq", lambda a: _seq(a, rev=True))

    def stub(name):
        def f(p, j, x, *rest):
            seen.append((name, rest))
            return dict(indptr=p, indices=j, values=x)
        return f
    for name in AM.ORDER:
        monkeypatch.setattr(G, name, stub(name))
    monkeypatch.setattr(G, "copy_csr_rows_numeric", stub("copy_csr_rows_numeric"))
    return seen


def matrix(dimnames=False):
    p = np.array([0, 2, 2, 5, 6, 6, 8], dtype=np.int32)
    j = np.array([0, 3, 1, 2, 4, 0, 1, 4], dtype=np.int32)
    dn = [list("abcdef"), list("vwxyz")] if dimnames else None
    return mx.dgRMatrix(p, j, np.arange(1.0, 9.0), (6, 5), dn)


def plain(rest):
    return tuple(a.tolist() if isinstance(a, np.ndarray) else a for a in rest)


# (i, j) 1-based as assign_csr takes them; the export's name without its _to_zero / _to_const ending; the arguments
# of the zero export; those of the const export with V standing for the value
V = "V"
SHAPES = [
    ([3], None, "set_single_row", (2,), (5, 2, V)),
    ([2, 3, 4], None, "set_rowseq", (1, 3), (1, 3, 5, V)),
    ([4, 3, 2], None, "set_rowseq", (1, 3), (1, 3, 5, V)),
    ([5, 1, 3], None, "set_arbitrary_rows", ([4, 0, 2],), ([4, 0, 2], 5, V)),
    (None, [4], "set_single_col", (3,), (5, 3, V)),
    (None, [2, 3], "set_colseq", (1, 2, 5), (1, 2, 5, V)),
    (None, [5, 4, 3], "set_colseq", (2, 4, 5), (2, 4, 5, V)),
    (None, [5, 1], "set_arbitrary_cols", ([4, 0], 5), ([4, 0], 5, V)),
    ([6], [1], "set_single_val", (5, 0), (5, 5, 0, V)),
    ([6, 2], [3], "set_arbitrary_rows_single_col", ([5, 1], 2, 5), ([5, 1], 2, V, 5)),
    ([1, 2, 3], [3], "set_arbitrary_rows_single_col", ([0, 1, 2], 2, 5), ([0, 1, 2], 2, V, 5)),
    ([2], [5, 2], "set_single_row_arbitrary_cols", (1, [4, 1], 5), (1, [4, 1], 5, V)),
    ([2], [1, 2], "set_single_row_arbitrary_cols", (1, [0, 1], 5), (1, [0, 1], 5, V)),
    ([6, 2], [5, 2], "set_arbitrary_rows_arbitrary_cols", ([5, 1], [4, 1], 5), ([5, 1], [4, 1], 5, V)),
    ([1, 2], [2, 3], "set_arbitrary_rows_arbitrary_cols", ([0, 1], [1, 2], 5), ([0, 1], [1, 2], 5, V)),
    ([True, False, False, False, False, True], None, "set_arbitrary_rows", ([0, 5],), ([0, 5], 5, V)),
    ([-1, -2, -3, -4, -5], None, "set_single_row", (5,), (5, 5, V)),
    (["b"], ["x", "v"], "set_single_row_arbitrary_cols", (1, [2, 0], 5), (1, [2, 0], 5, V)),
]


@pytest.mark.parametrize("i, j, stem, zero_args, const_args", SHAPES)
def test_every_selector_shape_reaches_its_export(calls, i, j, stem, zero_args, const_args):
    X = matrix(dimnames=True)
    for value in (0, 0.0, -0.0, np.zeros(1), np.array([[0]]), False, mx.float32(np.zeros(1, dtype=np.float32))):
        del calls[:]
        out = mx.assign_csr(X, i, j, value)
        assert [(n, plain(r)) for n, r in calls] == [(stem + "_to_zero", zero_args)], value
        assert isinstance(out, mx.dgRMatrix) and out is not X and out.Dimnames == X.Dimnames and out.Dim == X.Dim
    for value, sent in ((2.5, 2.5), (3, 3.0), (True, 1.0), (np.float32(0.5), 0.5), (np.array([7.0]), 7.0)):
        del calls[:]
        mx.assign_csr(X, i, j, value)
        want = tuple(sent if a is V else a for a in const_args)
        assert [(n, plain(r)) for n, r in calls] == [(stem + "_to_const", want)], value
    for value in (NA, np.int32(mx.NA_INTEGER), np.array([mx.NA_LOGICAL], dtype=np.int32)):   # NA of any type: NA_real_
        del calls[:]
        mx.assign_csr(X, i, j, value)
        (name, rest), = calls
        sent = rest[AM.ORDER[name].index("val")]
        assert name == stem + "_to_const" and np.float64(sent).view(np.uint64) == 0x7FF00000000007A2


def test_all_rows_and_all_columns_stay_on_the_host(calls):
    X = matrix(dimnames=True)
    out = mx.assign_csr(X, None, None, 0)
    assert isinstance(out, mx.dgRMatrix) and out.p.tolist() == [0] * 7 and out.j.size == 0 and out.x.size == 0
    assert out.Dim == (6, 5) and out.Dimnames == X.Dimnames and X.j.size == 8
    with pytest.warns(UserWarning, match=r"^Warning: attempting to set all coordinates in a sparse matrix\.$"):
        out = mx.assign_csr(X, np.arange(1, 7), [1, 2, 3, 4, 5], 2.5)
    assert isinstance(out, mx.DenseMatrix) and out.shape == (6, 5) and np.all(np.asarray(out) == 2.5)
    assert out.Dimnames == X.Dimnames
    with pytest.warns(UserWarning):
        out = mx.assign_csr(X, None, None, NA)
    assert np.all(np.asarray(out).view(np.uint64) == 0x7FF00000000007A2)
    assert calls == []
    with pytest.raises(mx.MatrixExtraError, match="assign_csr"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        X[:, :] = 1.0
    X[:, :] = 0
    assert X.j.size == 0 and X.p.tolist() == [0] * 7


def test_setitem_uses_zero_based_keys_and_rebinds(calls, monkeypatch):
    X = matrix()
    X[2, :] = 0
    X[[5, 1], 2] = 4.0
    X[1:4] = 0
    X[:, -1] = 1.0
    assert [(n, plain(r)) for n, r in calls] == [
        ("set_single_row_to_zero", (2,)), ("set_arbitrary_rows_single_col_to_const", ([5, 1], 2, 4.0, 5)),
        ("set_rowseq_to_zero", (1, 3)), ("set_single_col_to_const", (5, 4, 1.0))]
    new = dict(indptr=np.zeros(7, dtype=np.int32), indices=np.zeros(0, dtype=np.int32), values=np.zeros(0))
    monkeypatch.setattr(G, "set_single_row_to_zero", lambda *a: new)
    X[0, :] = 0
    assert X.p is not None and X.j.size == 0 and X.x.size == 0 and X.Dim == (6, 5)


def test_messages_of_the_reference(calls):
    X = matrix()
    for bad in (None, "text", [1.0, 2.0], np.zeros(0), np.zeros((0, 3)), {"a": 1}, mx.dsparseVector([], [], 0)):
        with pytest.raises(mx.MatrixExtraError, match=r"^Invalid value to assign\.$"):
            mx.assign_csr(X, [1], None, bad)
    for i, j in (([1, mx.NA_INTEGER], None), (None, np.array([1.0, np.nan])), ([2, None], [1])):
        with pytest.raises(mx.MatrixExtraError, match=r"^Indices contain NAs\.$"):
            mx.assign_csr(X, i, j, 0)
    shape = r"^Values to assign do not match with matrix dimensions\.$"
    with pytest.raises(mx.MatrixExtraError, match=shape):
        mx.assign_csr(X, [1], None, np.ones(3))                          # 5 columns, 3 values
    with pytest.raises(mx.MatrixExtraError, match=shape):
        mx.assign_csr(X, None, [2], np.ones(4))                          # 6 rows, 4 values
    with pytest.raises(mx.MatrixExtraError, match=shape):
        mx.assign_csr(X, [1, 2], [1, 2, 3], np.ones(4))
    with pytest.raises(mx.MatrixExtraError, match=shape):
        mx.assign_csr(X, None, None, np.ones(7))
    with pytest.raises(mx.MatrixExtraError, match=shape):                # an empty sparse value is checked, then is 0
        mx.assign_csr(X, [1, 2], None, mx.dgRMatrix(np.zeros(4, dtype=np.int32), [], [], (3, 5)))
    with pytest.raises(mx.MatrixExtraError, match=shape):
        mx.assign_csr(X, [1, 2], [1, 2], mx.dsparseVector([], [], 3))
    with pytest.raises(mx.MatrixExtraError, match=shape):                # whole rows wanted: 2 rows selected, 3 given
        mx.assign_csr(X, [5, 1], None, mx.dgRMatrix([0, 1, 1, 2], [0, 1], [1.0, 2.0], (3, 5)))
    assert calls == []


def test_routes_the_reference_sends_elsewhere_are_refused(calls):
    X = matrix()
    sv = mx.dsparseVector([2], [1.5], 5)
    sm = mx.dgRMatrix([0, 1, 2], [0, 1], [1.0, 2.0], (2, 2))
    cases = [
        (([1, 1], None, 0), "duplicated indices"), ((None, [2, 2], 1.0), "duplicated indices"),
        (([1], None, np.ones(5)), "set_single_row_to_rowvec"), ((None, [2], np.ones(6)), "set_single_col_to_colvec"),
        (([1, 2], None, np.ones(10)), "vector value"), (([1, 2], [1, 2], np.ones((2, 2))), "vector value"),
        ((None, None, np.ones(30)), "vector"),
        (([1], None, sv), "set_single_row_to_svec"), ((None, [1], mx.dsparseVector([2], [1.5], 6)), "set_single_col_to_svec"),
        (([1, 2], None, sv), "sparseVector value"),
        (([1, 2], [1, 2], sm), "sparse matrix value"), ((None, [1, 2], sm), "sparse matrix value"),
        (([1, 2], None, mx.dgRMatrix([0, 1], [0], [1.0], (1, 5))), "not whole rows"),
        (([1], None, mx.dgRMatrix([0, 1], [0], [1.0], (1, 5))), "set_single_row_to_svec"),
    ]
    for (i, j, value), route in cases:
        with pytest.raises(mx.MatrixExtraError, match="not on the device") as e:
            mx.assign_csr(X, i, j, value)
        assert route in str(e.value), (route, str(e.value))
    assert calls == []
    with pytest.raises(mx.MatrixExtraError, match="dgRMatrix"):
        mx.assign_csr(mx.lgRMatrix(X.p, X.j, np.ones(8, dtype=np.int32), X.Dim), [1], None, 0)


def test_sparse_values_without_entries_and_of_one_cell_are_scalars(calls):
    X = matrix()
    mx.assign_csr(X, [1, 2], None, mx.dgRMatrix(np.zeros(3, dtype=np.int32), [], [], (2, 5)))
    mx.assign_csr(X, [2], [1, 3], mx.dsparseVector([], [], 2))
    mx.assign_csr(X, [2], [1, 3], mx.dsparseVector([1], [4.0], 1))
    mx.assign_csr(X, [3], None, mx.dgRMatrix([0, 1], [0], [6.0], (1, 1)))
    assert [(n, plain(r)) for n, r in calls] == [
        ("set_rowseq_to_zero", (0, 1)), ("set_single_row_arbitrary_cols_to_zero", (1, [0, 2], 5)),
        ("set_single_row_arbitrary_cols_to_const", (1, [0, 2], 5, 4.0)), ("set_single_row_to_const", (5, 2, 6.0))]


def test_row_replacement_routes(calls, monkeypatch):
    X = matrix(dimnames=True)
    V3 = mx.dgRMatrix([0, 1, 1, 3], [4, 0, 2], [1.0, 2.0, 3.0], (3, 5))
    mx.assign_csr(X, [2, 3, 4], None, V3)
    mx.assign_csr(X, [4, 3, 2], None, V3)                    # rev-seq: the selector goes to the device as given
    mx.assign_csr(X, [6, 1, 3], None, V3)
    names = [n for n, _ in calls]
    assert names == ["set_rowseq_to_smat", "set_arbitrary_rows_to_smat", "set_arbitrary_rows_to_smat"]
    assert plain(calls[0][1][:2]) == (1, 3) and calls[0][1][2] is V3.p and calls[0][1][4] is V3.x
    assert plain(calls[1][1][:1]) == ([3, 2, 1],) and plain(calls[2][1][:1]) == ([5, 0, 2],)
    # a permutation of all rows is the gather of the value alone (R/assignment.R:430-431)
    del calls[:]
    V6 = mx.dgRMatrix(np.arange(7, dtype=np.int32), np.zeros(6, dtype=np.int32), np.arange(6.0), (6, 5))
    mx.assign_csr(X, [3, 1, 2, 6, 5, 4], None, V6)
    assert [(n, plain(r)) for n, r in calls] == [("copy_csr_rows_numeric", ([1, 2, 0, 5, 4, 3],))]
    # all rows and all columns with a value of the same shape: the value as a CSR (:361-362)
    assert mx.assign_csr(X, None, None, V6.copy()).x.tolist() == V6.x.tolist()


def test_rows_that_are_not_sorted_are_sorted_in_a_copy(calls, monkeypatch):
    X = matrix()
    X.j[2:5] = [4, 1, 2]
    sorted_copy = []

    def fake_sort(Y, copy=False, byrow=True):
        assert copy and Y is X
        Z = Y.copy()
        Z.j[2:5] = [1, 2, 4]
        sorted_copy.append(Z)
        return Z
    monkeypatch.setattr(A, "sort_sparse_indices", fake_sort)
    assert not G.rows_are_sorted(X.p, X.j)
    mx.assign_csr(X, [1], None, 1.0)
    mx.assign_csr(X, None, [2], 0)
    assert len(sorted_copy) == 2 and X.j[2:5].tolist() == [4, 1, 2]
    assert G.rows_are_sorted(np.array([0, 2, 2, 3]), np.array([1, 5, 0])) and G.rows_are_sorted([0, 0], [])
    assert not G.rows_are_sorted(np.array([0, 2, 3]), np.array([1, 1, 0]))


def test_export_helpers_refuse_before_any_device_call():
    p, j, x = np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2)
    with pytest.raises(ValueError):
        G.set_single_row_to_zero(p, j, np.ones(3), 0)
    cases = [
        (lambda: G.set_single_row_to_zero(p, j, x, 2), "row index 2 outside"),
        (lambda: G.set_single_col_to_const(p, j, x, 2, 2, 1.0), "column index 2 outside"),
        (lambda: G.set_rowseq_to_zero(p, j, x, 1, 0), "lo 1 > hi 0"),
        (lambda: G.set_colseq_to_zero(p, j, x, 0, 2, 2), "outside"),
        (lambda: G.set_arbitrary_rows_to_zero(p, j, x, [0, 5]), "row index 5 outside"),
        (lambda: G.set_arbitrary_cols_to_zero(p, j, x, [1, 1], 2), "duplicates"),
        (lambda: G.set_rowseq_to_smat(p, j, x, 0, 1, np.array([0, 1], dtype=np.int32), j[:1], x[:1]), "rows"),
        (lambda: G.set_arbitrary_rows_to_smat(p, j, x, [1], np.array([0, 1, 2], dtype=np.int32), j, x), "rows"),
    ]
    for call, text in cases:
        with pytest.raises(mx._lib.MxError, match=text):
            call()


def test_the_r_side_carries_the_same_names():
    import rshim_registry
    with open(os.path.join(ROOT, "include", "mxgpu.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "matrixextra_amd", "csrc", "r_shim.cpp")) as f:
        shim = f.read()
    for name in AM.ORDER:
        rshim_registry.assert_shim_and_overlay_carry(name, 3 + len(AM.ORDER[name]))     # registered, exported, rebound
        assert callable(getattr(G, name))
    assert "mx_assign_csr_scalar_begin" in shim and "mx_assign_csr_rows_begin" in shim
    for proto in ("mx_assign_csr_scalar_begin", "mx_assign_csr_rows_begin"):
        before = header[:header.index("int " + proto)]
        assert "src/assignment.cpp:" in before[before.rindex("/*"):], proto
    assert mx.assign_csr is A.assign_csr
