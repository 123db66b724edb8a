"""What `matrix * sparseVector` and the COO * matrix route decide before a device call: the C-ABI symbols and the
route rule, the arguments the C-ABI refuses before any launch, and the dispatch of the Python mirror
(R/operators.R:400-483, 1641-1705) with the exports replaced.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G, matrices, operators

MX_SYMBOLS = ["mx_dense_by_svec_route", "mx_multiply_elemwise_dense_by_svec_begin",
              "mx_multiply_elemwise_dense_by_svec_dense", "mx_multiply_coo_by_dense_numeric",
              "mx_multiply_coo_by_dense_integer", "mx_multiply_coo_by_dense_logical", "mx_multiply_coo_by_dense_float32",
              "mx_logicaland_coo_by_dense_logical"]
MXD_SYMBOLS = ["mxd_dense_by_svec_count", "mxd_dense_by_svec_fill", "mxd_dense_by_svec_dense", "mxd_coo_by_dense"]
SVEC_EXPORTS = ["multiply_elemwise_dense_by_svec_" + k for k in ("numeric", "integer", "logical", "float32")]
COO_EXPORTS = ["multiply_coo_by_dense_" + k for k in ("numeric", "integer", "logical", "float32")] + \
              ["logicaland_coo_by_dense_logical"]
OPTION = "mxgpu.coo_dense_route"


@pytest.mark.parametrize("name", MX_SYMBOLS + MXD_SYMBOLS + ["mxd_dense_by_svec_workspace_bytes"])
def test_symbol_is_declared_and_bound(name):
    assert name in _lib.declared_symbols()
    fn = getattr(_lib.load(), name)
    assert fn.argtypes == _lib.HEADER.functions[name][1]


def test_abi_version_stays():
    assert _lib.MXGPU_ABI_VERSION == 1 and _lib.load().mx_abi_version() == 1


@pytest.mark.parametrize("name", SVEC_EXPORTS + COO_EXPORTS)
def test_export_exists_under_the_reference_name(name):
    assert callable(getattr(G, name))


def test_route_follows_the_table():
    A, B, Cr, D = (_lib.MX_DSV_ROUTE_A, _lib.MX_DSV_ROUTE_B, _lib.MX_DSV_ROUTE_C, _lib.MX_DSV_ROUTE_D)
    assert (A, B, Cr, D) == (0, 1, 2, 3)
    r = G.dense_by_svec_route
    assert r(65, 2, 130) == A and r(65, 2, 65) == B and r(65, 2, 13) == Cr and r(65, 2, 5) == Cr
    assert r(65, 2, 7) == D and r(65, 2, 68) == D and r(65, 2, 1) == Cr
    assert r(63, 1, 63) == A                                 # one column: route A wins the tie with route B
    assert r(1, 64, 64) == A and r(1, 64, 1) == B and r(1, 1, 1) == A
    assert r(46341, 46341, 46341) == B                       # the cell count is taken in 64 bits
    assert r(0, 5, 0) == A and r(0, 5, 3) == D and r(4, 0, 4) == B
    for bad in ((-1, 2, 2), (2, -1, 2), (2, 2, -1), (2, 2, 0)):
        with pytest.raises(_lib.MxError, match="mx_dense_by_svec_route"):
            r(*bad)


def test_the_vector_is_checked_against_its_length_before_any_launch():
    X = np.asfortranarray(np.arange(12.0).reshape(6, 2))
    for length in (6, 3, 12, 5):                             # routes B, C, A, D
        for ii in ([0], [length + 1], [1, -3]):
            with pytest.raises(_lib.MxError, match=rf"lies outside 1\.\.{length}"):
                G.multiply_elemwise_dense_by_svec_numeric(X, np.array(ii, dtype=np.int32), np.ones(len(ii)), length, 1)
    with pytest.raises(_lib.MxError, match="more than its length 3"):
        G.multiply_elemwise_dense_by_svec_integer(X.astype(np.int32), np.array([1, 2, 3, 1], dtype=np.int32), np.ones(4), 3, 0)
    with pytest.raises(ValueError, match="different lengths"):
        G.multiply_elemwise_dense_by_svec_numeric(X, np.array([1, 2], dtype=np.int32), np.ones(1), 6, 1)
    with pytest.raises(ValueError, match="2-d"):
        G.multiply_elemwise_dense_by_svec_numeric(np.ones(6), np.array([1], dtype=np.int32), np.ones(1), 6, 1)


def test_each_entry_refuses_the_other_routes():
    lib = _lib.load()
    X = np.asfortranarray(np.arange(12.0).reshape(6, 2))
    ii, xx, out = np.array([1], dtype=np.int32), np.ones(1), np.empty((6, 2), order="F")
    res, info = C.c_void_p(), _lib.ResultInfo()
    for length in (12, 5):
        assert lib.mx_multiply_elemwise_dense_by_svec_begin(_lib.ptr(X), 0, 6, 2, _lib.ptr(ii), _lib.ptr(xx), 1, length, 1,
                                                            C.byref(res), C.byref(info)) != 0
        assert "gives a dense result" in lib.mx_last_error().decode() and not res.value
    for length in (6, 3):
        assert lib.mx_multiply_elemwise_dense_by_svec_dense(_lib.ptr(X), 0, 6, 2, _lib.ptr(ii), _lib.ptr(xx), 1, length, 1,
                                                            _lib.ptr(out)) != 0
        assert "gives a CSR result" in lib.mx_last_error().decode()
    assert lib.mx_multiply_elemwise_dense_by_svec_dense(_lib.ptr(X), 4, 6, 2, _lib.ptr(ii), _lib.ptr(xx), 1, 12, 1,
                                                        _lib.ptr(out)) != 0
    assert "bad arguments" in lib.mx_last_error().decode()


@pytest.mark.parametrize("name", COO_EXPORTS)
def test_coo_entries_outside_the_matrix_are_refused(name):
    dt = np.float32 if name.endswith("float32") else np.float64 if name.endswith("numeric") else np.int32
    X = np.asfortranarray(np.ones((4, 3), dtype=dt))
    xx = np.ones(2, dtype=np.int32 if name.startswith("logicaland") else np.float64)
    for ii, jj in (([0, 4], [0, 0]), ([0, 1], [3, 0]), ([-1, 1], [0, 0]), ([0, 1], [0, -2])):
        with pytest.raises(_lib.MxError, match="lies outside the 4 x 3 matrix"):
            getattr(G, name)(X, np.array(ii, dtype=np.int32), np.array(jj, dtype=np.int32), xx)
    with pytest.raises(ValueError, match="different lengths"):
        getattr(G, name)(X, np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), xx)
    empty = np.zeros(0, dtype=np.int32)
    res = getattr(G, name)(X, empty, empty, xx[:0])           # nothing stored: nothing reaches the device
    assert res["val"].size == 0 and res["val"].dtype == xx.dtype and res["row"] is not empty


# ----------------------------------------------------------------------------- the mirror, exports replaced
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def svec(name):
        def f(X, ii, xx, length, keep):
            seen.append((name, X, ii, xx, length, keep))
            if G.dense_by_svec_route(X.shape[0], X.shape[1], length) in (0, 3):
                return dict(X_dense=np.full(X.shape, 7.0, order="F"))
            return dict(indptr=np.zeros(X.shape[0] + 1, np.int32), indices=np.zeros(0, np.int32), values=np.zeros(0))
        return f

    def coo(name):
        def f(X, row, col, val):
            seen.append((name, X, row, col, val))
            return dict(row=row.copy(), col=col.copy(), val=np.asarray(val) * 2)
        return f

    for name in SVEC_EXPORTS:
        monkeypatch.setattr(G, name, svec(name))
    for name in COO_EXPORTS:
        monkeypatch.setattr(G, name, coo(name))

    def sort_vec(i, x=None):
        seen.append(("sort", i))
        o = np.argsort(i, kind="stable")
        i[:] = i[o]
        if x is not None:
            x[:] = x[o]
    for k in ("numeric", "integer", "logical"):
        monkeypatch.setattr(G, "sort_vector_indices_" + k, sort_vec)
    return seen


def test_svec_times_anything_but_a_matrix_is_not_implemented():
    v = mx.dsparseVector([1, 3], [2.0, 4.0], 4)
    assert v.__mul__(np.ones(4)) is NotImplemented and v.__rmul__(np.ones(4)) is NotImplemented
    assert v.__mul__(2.0) is NotImplemented and v.__rmul__(2.0) is NotImplemented
    assert v.__mul__(np.ones((2, 2, 1))) is NotImplemented
    assert v.__mul__(mx.dgRMatrix([0, 1], [0], [1.0], (1, 1))) is NotImplemented
    with pytest.raises(TypeError):
        np.ones(4) * v


def test_matrix_times_svec_dispatch(calls, monkeypatch):
    v = mx.dsparseVector([3, 1], [2.0, 4.0], 4)
    M = mx.DenseMatrix(np.arange(8.0).reshape(4, 2), [["a", "b", "c", "d"], None])
    out = M * v                                               # route B: a dgRMatrix with M's Dim and Dimnames
    name, X, ii, xx, length, keep = calls[-1]
    assert name.endswith("_numeric") and length == 4 and keep is True
    assert ii.tolist() == [1, 3] and xx.tolist() == [4.0, 2.0]            # sorted, in a copy
    assert v.i.tolist() == [3, 1] and calls[0][0] == "sort"
    assert isinstance(out, mx.dgRMatrix) and out.Dim == (4, 2) and out.Dimnames == [["a", "b", "c", "d"], None]
    out = v * M
    assert isinstance(out, mx.dgRMatrix) and calls[-1][0].endswith("_numeric")

    monkeypatch.setitem(matrices.options, "MatrixExtra.inplace_sort", True)
    M * v
    assert v.i.tolist() == [1, 3] and calls[-1][2] is v.i                 # a dsparseVector is sorted in place
    w = mx.isparseVector([2, 1], [5, 6], 4)
    M * w                                                                 # another kind is copied, then converted
    assert w.i.tolist() == [2, 1] and calls[-1][2].tolist() == [1, 2] and calls[-1][3].tolist() == [6.0, 5.0]
    monkeypatch.setitem(matrices.options, "MatrixExtra.inplace_sort", False)

    monkeypatch.setitem(matrices.options, "MatrixExtra.ignore_na", True)
    u = mx.dsparseVector([3, 1], [2.0, 4.0], 4)
    n_sorts = sum(c[0] == "sort" for c in calls)
    M * u                                                                 # no sort when NAs are ignored
    assert sum(c[0] == "sort" for c in calls) == n_sorts and calls[-1][2].tolist() == [3, 1] and calls[-1][5] is False
    monkeypatch.setitem(matrices.options, "MatrixExtra.ignore_na", False)

    out = M * mx.dsparseVector([8], [1.0], 8)                             # route A: the dense matrix as it is
    assert isinstance(out, np.ndarray) and not hasattr(out, "p") and out.shape == (4, 2) and (out == 7.0).all()
    out = M * mx.dsparseVector([1], [1.0], 3)                             # route D
    assert isinstance(out, np.ndarray) and out.shape == (4, 2)


def test_matrix_kinds_reach_their_exports(calls):
    v = mx.dsparseVector([1], [2.0], 4)
    for M, suffix, dt in ((np.ones((4, 2), dtype=np.int32), "_integer", np.int32), (np.ones((4, 2), dtype=bool), "_logical", np.bool_),
                          (np.ones((4, 2)), "_numeric", np.float64), (np.ones((4, 2), dtype=np.int64), "_numeric", np.float64),
                          (np.ones((4, 2), dtype=np.float32), "_numeric", np.float64)):
        M * v
        assert calls[-1][0].endswith(suffix) and calls[-1][1].dtype == dt
    f = mx.float32(np.ones((4, 2), dtype=np.float32), [None, ["x", "y"]])
    for out in (f * v, v * f):
        assert calls[-1][0].endswith("_float32") and calls[-1][1].dtype == np.float32
        assert isinstance(out, mx.dgRMatrix) and out.Dim == (4, 2) and out.Dimnames == [None, ["x", "y"]]
    mx.float32(np.ones(4, dtype=np.float32)) * v                          # a float32 vector is a one-column matrix
    assert calls[-1][1].shape == (4, 1)


def test_empty_operands_give_the_one_cell_matrix(calls):
    for out in (np.ones((0, 3)) * mx.dsparseVector([1], [2.0], 4), np.ones((2, 3)) * mx.dsparseVector([], [], 0)):
        assert out.shape == (1, 1) and np.isnan(out[0, 0])
    assert not calls


def test_coo_route_is_inert_without_the_option(monkeypatch):
    assert not matrices.options.get(OPTION, False)
    for name in COO_EXPORTS:
        monkeypatch.setattr(G, name, lambda *a: pytest.fail("a COO * dense export was reached without the option"))
    seen = []
    monkeypatch.setattr(operators, "csr_op_vector", lambda e1, e2, op, X_is_LHS=True: seen.append((op, e2)) or "vector route")
    T = mx.dgTMatrix([0, 1], [1, 0], [2.0, 3.0], (2, 2))
    D = np.array([[1, 2], [3, 4]], dtype=np.int32)
    assert T * D == "vector route" and D * T == "vector route" and (T & D) == "vector route" and (D & T) == "vector route"
    assert [op for op, _ in seen] == ["*", "*", "&", "&"] and all(e2 is D for _, e2 in seen)


def test_coo_route_under_the_option(calls, monkeypatch):
    monkeypatch.setitem(matrices.options, OPTION, True)
    vec = []
    monkeypatch.setattr(operators, "multiply_csr_by_dvec_elemwise_internal",
                        lambda e1, e2, logical=False, **k: vec.append((e2.dtype, logical)) or "vector route")
    csc = []
    monkeypatch.setattr(operators, "multiply_csc_by_dense_internal", lambda e1, e2, logical=False: csc.append(type(e1)) or "csc route")
    monkeypatch.setattr(operators, "as_csc_matrix", lambda e1: "csc")
    T = mx.dgTMatrix([0, 1], [1, 0], [2.0, 3.0], (2, 2))
    Di = np.array([[1, 2], [3, 4]], dtype=np.int32)
    for out in (T * Di, Di * T):
        assert calls[-1][0] == "multiply_coo_by_dense_integer" and calls[-1][1] is Di
        assert isinstance(out, mx.dgTMatrix) and out.Dim == (2, 2) and out.x.tolist() == [4.0, 6.0]
        assert out.i is not T.i and out.i.tolist() == [0, 1]
    T * np.array([[True, False], [True, True]])
    assert calls[-1][0] == "multiply_coo_by_dense_logical"
    n = len(calls)
    assert T * np.ones((2, 2)) == "vector route" and vec[-1] == (np.float64, False)      # :402-403
    assert (T & Di) == "vector route" and vec[-1][1] is True                             # every `&`, too
    L = mx.lgTMatrix([0, 1], [1, 0], [1, mx.NA_LOGICAL], (2, 2))
    assert (L & np.array([[True, False], [True, True]])) == "vector route" and vec[-1][1] is True
    Dna = np.array([[1, mx.NA_INTEGER], [3, 4]], dtype=np.int32)
    assert T * Dna == "csc route" and csc == [str]                                       # :412-415
    monkeypatch.setitem(matrices.options, "MatrixExtra.ignore_na", True)
    T * Dna
    assert calls[-1][0] == "multiply_coo_by_dense_integer" and len(calls) == n + 1
    monkeypatch.setitem(matrices.options, "MatrixExtra.ignore_na", False)
    with pytest.raises(mx.MatrixExtraError, match="dimensions do not match"):
        T * np.ones((1, 2), dtype=np.int32)
    with pytest.raises(mx.MatrixExtraError, match="Unexpected error"):                   # the float32 branch, :455-464
        T * mx.float32(np.ones((2, 2), dtype=np.float32))
    assert len(calls) == n + 1
