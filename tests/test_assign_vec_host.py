"""Host side of the vector-valued CSR assignment, no device call: the four exports with the
reference's arities, the C-ABI symbols, every export-level check with its message, and the mirror
(matrixextra_amd/assign.py) with the native routines stubbed: unchanged refusals without
options["mxgpu.assign_vec_route"], and under it the export each value reaches, with which arguments."""
import inspect
import json
import os

import numpy as np
import pytest

import assign_vec_model as VM
import matrixextra_amd as mx
from matrixextra_amd import _lib, matrices
from matrixextra_amd import assign as A
from matrixextra_amd import exports as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "mxgpu.assign_vec_route"
SHAPE = r"^Values to assign do not match with matrix dimensions\.$"


def test_exports_carry_the_reference_arities():
    with open(os.path.join(ROOT, "tests", "golden", "call_signatures.json")) as f:
        sigs = json.load(f)
    for name, rest in VM.ORDER.items():
        params = list(inspect.signature(getattr(G, name)).parameters)
        assert len(params) == sigs[name]["arity"] == 3 + len(rest), name
        assert params[:3] == ["indptr", "indices", "values"] and params[3] == "ncols", name
    assert list(inspect.signature(G.set_single_row_to_svec).parameters)[4:] == ["row_set", "ii", "xx", "length"]
    assert list(inspect.signature(G.set_single_col_to_colvec).parameters)[4:] == ["col_set", "vec_set"]


def test_symbols_are_declared_where_they_belong():
    names = set(_lib.declared_symbols())
    wanted = {"mxd_csr_assign_col_count", "mxd_csr_assign_col_fill", "mxd_csr_expand_pattern_row",
              "mx_assign_csr_row_vec_begin", "mx_assign_csr_col_vec_begin"}
    assert wanted <= names
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in wanted)
    assert len(_lib.HEADER.functions["mx_assign_csr_row_vec_begin"][1]) == 12
    assert _lib.HEADER.functions["mx_assign_csr_row_vec_begin"] == _lib.HEADER.functions["mx_assign_csr_col_vec_begin"]
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for proto in wanted:                                   # each cites the reference lines it replaces
        before = header[:header.index("int " + proto)]
        assert "src/assignment.cpp:" in before[before.rindex("/*"):], proto
    csrc = os.path.join(ROOT, "matrixextra_amd", "csrc")
    with open(os.path.join(csrc, "api.hip")) as f:
        assert "mx_assign_csr_" not in f.read()
    with open(os.path.join(csrc, "api_assign.hip")) as f:
        text = f.read()
    assert "mx_assign_csr_row_vec_begin" in text and "mx_assign_csr_col_vec_begin" in text
    with open(os.path.join(csrc, "Makefile")) as f:
        assert " assignvec.hip " in f.read()
    # no workspace function of its own: the count block of the gathers
    assert not any("assign" in n and n.endswith("_workspace_bytes") for n in names)


def test_export_checks_refuse_before_any_device_call():
    p, j, x = np.array([0, 1, 2, 2, 3], dtype=np.int32), np.array([0, 1, 5], dtype=np.int32), np.ones(3)
    i32 = lambda *a: np.array(a, dtype=np.int32)        # noqa: E731
    with pytest.raises(ValueError):
        G.set_single_row_to_rowvec(p, j, np.ones(2), 6, 0, np.ones(6))
    with pytest.raises(ValueError):
        G.set_single_row_to_svec(p, j, x, 6, 0, i32(0, 1), np.ones(1), 6)
    cases = [
        (lambda: G.set_single_row_to_rowvec(p, j, x, 6, 4, np.ones(6)), "row index 4 outside"),
        (lambda: G.set_single_row_to_rowvec(p, j, x, 6, -1, np.ones(6)), "row index -1 outside"),
        (lambda: G.set_single_col_to_colvec(p, j, x, 6, 6, np.ones(4)), "column index 6 outside"),
        (lambda: G.set_single_col_to_svec(p, j, x, 6, -1, i32(0), np.ones(1), 4), "column index -1 outside"),
        (lambda: G.set_single_row_to_rowvec(p, j, x, 6, 0, np.zeros(0)), "length 0 is not positive"),
        (lambda: G.set_single_row_to_svec(p, j, x, 6, 0, i32(0), np.ones(1), -2), "length -2 is not positive"),
        (lambda: G.set_single_row_to_rowvec(p, j, x, 6, 0, np.ones(4)), "length 4 does not divide the 6 columns"),
        (lambda: G.set_single_row_to_rowvec(p, j, x, 6, 0, np.ones(12)), "length 12 does not divide the 6 columns"),
        (lambda: G.set_single_col_to_colvec(p, j, x, 6, 0, np.ones(3)), "length 3 does not divide the 4 rows"),
        (lambda: G.set_single_col_to_svec(p, j, x, 6, 0, i32(0), np.ones(1), 8), "length 8 does not divide the 4 rows"),
        (lambda: G.set_single_row_to_svec(p, j, x, 6, 0, i32(0, 3), np.ones(2), 3), r"vector index 3 outside \[0, 3\)"),
        (lambda: G.set_single_col_to_svec(p, j, x, 6, 0, i32(-1), np.ones(1), 2), r"vector index -1 outside \[0, 2\)"),
        (lambda: G.set_single_col_to_svec(p, j, x, 6, 0, i32(1, 0), np.ones(2), 2), "not strictly ascending"),
        (lambda: G.set_single_col_to_svec(p, j, x, 6, 0, i32(1, 1), np.ones(2), 2), "not strictly ascending"),
        (lambda: G.set_single_row_to_svec(p, j, x, 6, 0, i32(0, 1, 0), np.ones(3), 2), "has 3 entries, its length is 2"),
    ]
    for call, text in cases:
        with pytest.raises(_lib.MxError, match=text):
            call()
    lib = _lib.load()
    info, res = _lib.ResultInfo(), __import__("ctypes").c_void_p()
    byref = __import__("ctypes").byref
    P, J, X, V = _lib.ptr(p), _lib.ptr(j), _lib.ptr(x), _lib.ptr(np.ones(6))
    for fn in (lib.mx_assign_csr_row_vec_begin, lib.mx_assign_csr_col_vec_begin):
        for args, text in (((P, 4, J, X, 6, 0, None, V, 6, 6, None, byref(info)), "null output pointer"),
                           ((None, 4, J, X, 6, 0, None, V, 6, 6, byref(res), byref(info)), "null index pointer"),
                           ((P, 4, None, X, 6, 0, None, V, 6, 6, byref(res), byref(info)), "null indices or values"),
                           ((P, -1, J, X, 6, 0, None, V, 6, 6, byref(res), byref(info)), "negative number of rows"),
                           ((P, 4, J, X, 6, 0, None, None, 2, 2, byref(res), byref(info)), "null values of the vector")):
            assert fn(*args) != 0
            assert text in lib.mx_last_error().decode(), (text, lib.mx_last_error().decode())


# ---- the mirror ------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """The four exports (and the device sort of a sparseVector) replaced by recorders that return their inputs."""
    seen = []
    seq = lambda a, step: bool(np.all(np.diff(np.asarray(a, dtype=np.int64)) == step))      # noqa: E731
    monkeypatch.setattr(G, "check_is_seq", lambda a: seq(a, 1))
    monkeypatch.setattr(G, "check_is_rev_seq", lambda a: seq(a, -1))

    def stub(name):
        def f(p, j, x, *rest):
            seen.append((name, rest))
            return dict(indptr=p, indices=j, values=x)
        return f
    for name in VM.ORDER:
        monkeypatch.setattr(G, name, stub(name))

    def sort_vector(ii, xx):                          # sort_vector_indices_numeric works in place
        o = np.argsort(ii, kind="stable")
        seen.append(("sort_vector_indices_numeric", ()))
        ii[:], xx[:] = ii[o], xx[o]
    monkeypatch.setattr(G, "sort_vector_indices_numeric", sort_vector)
    return seen


def matrix():
    p = np.array([0, 2, 2, 5, 6, 6, 8], dtype=np.int32)
    j = np.array([0, 3, 1, 2, 4, 0, 1, 4], dtype=np.int32)
    return mx.dgRMatrix(p, j, np.arange(1.0, 9.0), (6, 5), [list("abcdef"), list("vwxyz")])


def plain(rest):
    return tuple(a.tolist() if isinstance(a, np.ndarray) else a for a in rest)


def values():
    sv5, sv6 = mx.dsparseVector([4, 2], [1.5, 2.5], 5), mx.dsparseVector([5, 2], [1.5, 2.5], 6)
    row_m = mx.dgRMatrix([0, 2], [1, 3], [7.0, 8.0], (1, 5))                 # 1 x 5: positions 2 and 4
    col_m = mx.dgCMatrix([0, 2], [1, 4], [7.0, 8.0], (6, 1))                 # 6 x 1: positions 2 and 5
    col_m5 = mx.dgCMatrix([0, 2], [1, 4], [7.0, 8.0], (5, 1))                # 5 x 1 into a row: the reference's defect
    return sv5, sv6, row_m, col_m, col_m5


def test_without_the_option_every_route_refuses_as_before(calls):
    assert OPTION not in matrices.options
    X = matrix()
    sv5, sv6, row_m, col_m, col_m5 = values()
    for (i, j, value), route in [(([1], None, np.ones(5)), "set_single_row_to_rowvec"),
                                 ((None, [2], np.ones(6)), "set_single_col_to_colvec"),
                                 (([1], None, sv5), "set_single_row_to_svec"), ((None, [1], sv6), "set_single_col_to_svec"),
                                 (([1], None, row_m), "set_single_row_to_svec"), ((None, [1], col_m), "set_single_col_to_svec"),
                                 (([1], None, col_m5), "set_single_row_to_svec")]:
        with pytest.raises(mx.MatrixExtraError, match="not on the device") as e:
            mx.assign_csr(X, i, j, value)
        assert str(e.value) == f"This assignment takes the reference's route '{route}', which is not on the device."
    assert calls == []


def test_under_the_option_each_value_reaches_its_export(calls, monkeypatch):
    monkeypatch.setitem(matrices.options, OPTION, True)
    X = matrix()
    sv5, sv6, row_m, col_m, col_m5 = values()
    kept = [a.copy() for a in (X.p, X.j, X.x, sv5.i, sv5.x, sv6.i, sv6.x, row_m.j, col_m.i)]

    def one(i, j, value):
        del calls[:]
        out = mx.assign_csr(X, i, j, value)
        assert isinstance(out, mx.dgRMatrix) and out is not X and out.Dimnames == X.Dimnames and out.Dim == X.Dim
        return [(n, plain(r)) for n, r in calls]

    # dense vectors: as.numeric, recycled lengths, NA of any type
    assert one([3], None, np.arange(5.0)) == [("set_single_row_to_rowvec", (5, 2, [0.0, 1.0, 2.0, 3.0, 4.0]))]
    assert one(["f"], None, np.array([True, False, True, True, False])) == \
        [("set_single_row_to_rowvec", (5, 5, [1.0, 0.0, 1.0, 1.0, 0.0]))]
    assert one(None, [4], np.array([1, 2, 3], dtype=np.int32)) == [("set_single_col_to_colvec", (5, 3, [1.0, 2.0, 3.0]))]
    assert one(None, ["v"], np.ones((6, 1))) == [("set_single_col_to_colvec", (5, 0, [1.0] * 6))]
    one([2], None, np.array([1, mx.NA_INTEGER, 3, 4, 5], dtype=np.int32))
    assert VM.bits(calls[0][1][2])[1] == 0x7FF00000000007A2
    # sparseVector: the row route takes ii as stored, the column route sorts a copy first
    assert one([1], None, sv5) == [("set_single_row_to_svec", (5, 0, [3, 1], [1.5, 2.5], 5))]
    assert one(None, [2], sv6) == [("sort_vector_indices_numeric", ()),
                                   ("set_single_col_to_svec", (5, 1, [1, 4], [2.5, 1.5], 6))]
    assert one(None, [5], mx.dsparseVector([3], [9.0], 3)) == [("sort_vector_indices_numeric", ()),
                                                              ("set_single_col_to_svec", (5, 4, [2], [9.0], 3))]
    assert one([6], None, mx.isparseVector([5, 1], [mx.NA_INTEGER, 2], 5))[0][1][:2] == (5, 5)
    assert plain(calls[0][1][2:3]) == ([4, 0],) and VM.bits(calls[0][1][3])[0] == 0x7FF00000000007A2
    # a sparse matrix of one row or one column is the sparseVector it spells, with the vector's length
    assert one([4], None, row_m) == [("set_single_row_to_svec", (5, 3, [1, 3], [7.0, 8.0], 5))]
    assert one([4], None, col_m5) == [("set_single_row_to_svec", (5, 3, [1, 4], [7.0, 8.0], 5))]
    assert one(None, [3], col_m) == [("sort_vector_indices_numeric", ()),
                                     ("set_single_col_to_svec", (5, 2, [1, 4], [7.0, 8.0], 6))]
    assert one(None, [3], mx.dgRMatrix([0, 1], [2], [4.0], (1, 3))) == \
        [("sort_vector_indices_numeric", ()), ("set_single_col_to_svec", (5, 2, [2], [4.0], 3))]
    # neither x nor any value was changed
    now = (X.p, X.j, X.x, sv5.i, sv5.x, sv6.i, sv6.x, row_m.j, col_m.i)
    assert all(np.array_equal(a, b) for a, b in zip(now, kept))


def test_under_the_option_messages_and_other_refusals_stay(calls, monkeypatch):
    monkeypatch.setitem(matrices.options, OPTION, True)
    X = matrix()
    sv5, sv6, row_m, col_m, col_m5 = values()
    for i, j, value in (([1], None, np.ones(3)), ([1], None, np.ones(10)), (None, [2], np.ones(4)),
                        (None, [2], np.ones(12)), ([1], None, mx.dsparseVector([2], [1.0], 3)),
                        (None, [1], mx.dsparseVector([2], [1.0], 4)), ([1], None, mx.dgRMatrix([0, 1], [1], [1.0], (1, 3))),
                        (None, [1], mx.dgCMatrix([0, 1], [1], [1.0], (4, 1)))):
        with pytest.raises(mx.MatrixExtraError, match=SHAPE):          # the shape message comes first
            mx.assign_csr(X, i, j, value)
    cases = [(([1, 2], None, np.ones(10)), "vector value"), ((None, [1, 2], np.ones(12)), "vector value"),
             (([1, 2], [1, 2], np.ones(4)), "vector value"), ((None, None, np.ones(30)), "x[, ] <- vector"),
             (([1, 2], None, sv5), "sparseVector value"), ((None, None, mx.dsparseVector([2], [1.0], 30)), "sparseVector"),
             (([1], None, mx.nsparseVector([2, 3], None, 5)), "nsparseVector"),
             ((None, [2], mx.nsparseVector([2, 3], None, 6)), "nsparseVector"),
             ((None, [1, 2], row_m), "sparse matrix value"),
             (([1, 1], None, np.ones(5)), "duplicated indices")]
    for (i, j, value), route in cases:
        with pytest.raises(mx.MatrixExtraError, match="not on the device") as e:
            mx.assign_csr(X, i, j, value)
        assert route in str(e.value), (route, str(e.value))
    assert calls == []
    # scalars in disguise stay scalar assignments
    seen = []
    monkeypatch.setattr(G, "set_single_row_to_const", lambda p, j, x, *r: seen.append(r) or dict(indptr=p, indices=j, values=x))
    monkeypatch.setattr(G, "set_single_col_to_zero", lambda p, j, x, *r: seen.append(r) or dict(indptr=p, indices=j, values=x))
    mx.assign_csr(X, [1], None, mx.dsparseVector([1], [4.0], 1))
    mx.assign_csr(X, None, [2], mx.dsparseVector([], [], 3))
    assert seen == [(5, 0, 4.0), (1,)] and calls == []


def test_unsorted_rows_are_sorted_in_a_copy_for_the_column_routes_only(calls, monkeypatch):
    monkeypatch.setitem(matrices.options, OPTION, True)
    X = matrix()
    X.j[2:5] = [4, 1, 2]
    made = []

    def fake_sort(Y, copy=False, byrow=True):
        if isinstance(Y, mx.sparseVector):
            return Y.copy()
        assert copy and Y is X
        Z = Y.copy()
        Z.j[2:5] = [1, 2, 4]
        made.append(Z)
        return Z
    monkeypatch.setattr(A, "sort_sparse_indices", fake_sort)
    mx.assign_csr(X, [1], None, np.ones(5))
    mx.assign_csr(X, [1], None, mx.dsparseVector([2], [1.0], 5))
    assert made == []
    mx.assign_csr(X, None, [2], np.ones(6))
    mx.assign_csr(X, None, [2], mx.dsparseVector([2], [1.0], 6))
    assert len(made) == 2 and X.j[2:5].tolist() == [4, 1, 2]
