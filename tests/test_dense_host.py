"""The dense <-> compressed conversions before a device call: include/mxgpu_dense.h as the binding reads it, the failures
on bad arguments, device.dense_to_csr / csr_to_dense on the recording fake of tests/device_trace.py, and what the mirror
decides under options["mxgpu.dense_route"]: exports.dense_to_csr / csr_to_dense are replaced by the numpy model of
tests/dense_model.py, so no GPU is needed; without the option they are never reached."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_model as DM
import device_trace as T
import matrixextra_amd as mx
from dense_model import NA, bits
from matrixextra_amd import _lib, device as D, exports as G
from matrixextra_amd.matrices import options

NEW = ["mx_csr_to_dense", "mx_dense_to_csr_begin", "mxd_csr_to_dense", "mxd_dense_to_csr_count", "mxd_dense_to_csr_fill",
       "mxd_dense_to_csr_workspace_bytes"]
P, I, I64, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
F64, F32, I32, LGL, NONE = _lib.MX_F64, _lib.MX_F32, _lib.MX_I32, _lib.MX_LGL, _lib.MX_NONE
SYNC = {"mxd_dense_to_csr_workspace_bytes": None, "mxd_dense_to_csr_count": True, "mxd_dense_to_csr_fill": False,
        "mxd_csr_to_dense": False}


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_dense_header_parses_to_six_prototypes_bound_on_the_same_library():
    with open(_lib.DENSE_HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert sorted(h.functions) == NEW == sorted(_lib.DENSE_HEADER.functions)
    assert h.constants == {} and h.structs == {}
    assert h.functions["mxd_dense_to_csr_workspace_bytes"] == (SZ, (I, I, I, I))
    assert h.functions["mxd_dense_to_csr_count"] == (I, (I, I, P, I64, I, I, I, P, P, P, P))
    assert h.functions["mxd_dense_to_csr_fill"] == (I, (I, I, P, I64, I, I, I, P, P, P, P, I, P))
    assert h.functions["mxd_csr_to_dense"] == (I, (I, I, P, P, P, I, I, I, P, I64, I, P, P))
    assert h.functions["mx_dense_to_csr_begin"] == (I, (P, I, I, I, I, I, P, P))
    assert h.functions["mx_csr_to_dense"] == (I, (P, I, I, P, P, I, I, P, I))
    lib = _lib.load()
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)                                         # exported by libmxgpu.so
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name


def test_the_other_headers_keep_their_function_sets():
    others = (_lib.HEADER, _lib.REDUCE_HEADER, _lib.SYM_HEADER, _lib.TPROD_HEADER, _lib.SPGEMM_HEADER, _lib.GRAM_HEADER)
    assert not any(set(NEW) & set(h.functions) for h in others) and not set(NEW) & set(_lib.declared_symbols())
    assert sorted(_lib.GRAM_HEADER.functions) == ["mx_csr_gram_begin", "mxd_csr_spgemm_tri_count", "mxd_csr_spgemm_tri_fill"]
    assert sorted(_lib.SPGEMM_HEADER.functions) == ["mx_csr_spgemm_begin", "mxd_csr_spgemm_count", "mxd_csr_spgemm_fill",
                                                    "mxd_csr_spgemm_limits", "mxd_csr_spgemm_workspace_bytes"]
    assert sorted(_lib.TPROD_HEADER.functions) == ["mx_csr_tmatmul_dense", "mx_csr_tmatvec", "mxd_csr_transpose_by_order",
                                                   "mxd_segment_dot"]
    assert {"mxd_dense_to_svec_count", "mxd_dense_to_svec_fill", "mxd_entries_to_dense_vector"} <= set(_lib.declared_symbols())
    assert _lib.HEADER.constants["MXGPU_ABI_VERSION"] == _lib.load().mx_abi_version()


def test_every_device_prototype_states_its_synchronisation():
    with open(_lib.DENSE_HEADER_PATH) as f:
        text = f.read()
    assert {n for n in _lib.DENSE_HEADER.functions if n.startswith("mxd_")} == set(SYNC)
    for name, waits in SYNC.items():
        at = text.index(" %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == bool(waits), name
        assert ("no synchronisation" in comment) == (not waits), name
    at = text.index("int mxd_csr_to_dense(")
    assert "roles of m and n swapped" in text[text.rindex("/*", 0, at):at]      # CSR -> row-major dense is said there


def test_calls_fail_loudly_on_bad_arguments_before_any_device_work():
    lib = _lib.load()
    err = lambda: lib.mx_last_error().decode()                          # noqa: E731
    x = np.zeros(4)
    h = C.c_int64(0)
    count = lambda m, n, d, ld, dt, *rest: lib.mxd_dense_to_csr_count(m, n, d, ld, dt, 0, 0, *rest, None)   # noqa: E731
    assert count(-1, 2, _lib.ptr(x), 2, F64, _lib.ptr(x), _lib.ptr(x), C.byref(h)) != 0 and "negative dimension" in err()
    assert count(2, -2, _lib.ptr(x), 2, F64, _lib.ptr(x), _lib.ptr(x), C.byref(h)) != 0 and "negative dimension" in err()
    assert count(2, 2, _lib.ptr(x), 1, F64, _lib.ptr(x), _lib.ptr(x), C.byref(h)) != 0 and "ld 1 is smaller" in err()
    assert count(2, 2, _lib.ptr(x), 2, NONE, _lib.ptr(x), _lib.ptr(x), C.byref(h)) != 0 and "unsupported dense dtype" in err()
    assert count(2, 2, None, 2, F64, _lib.ptr(x), _lib.ptr(x), C.byref(h)) != 0 and "null pointer" in err()
    assert count(2, 2, _lib.ptr(x), 2, F64, None, _lib.ptr(x), C.byref(h)) != 0 and "null pointer" in err()
    assert count(2, 2, _lib.ptr(x), 2, F64, _lib.ptr(x), _lib.ptr(x), None) != 0 and "null pointer" in err()
    assert lib.mxd_dense_to_csr_count(2, 2, _lib.ptr(x), 2, F64, 0, -1, _lib.ptr(x), _lib.ptr(x), C.byref(h), None) != 0
    assert "col_splits" in err()
    fill = lambda m, n, ld, dt, odt, *ptrs: lib.mxd_dense_to_csr_fill(m, n, ptrs[0], ld, dt, 1, 0, *ptrs[1:5], odt, None)  # noqa: E731
    px = _lib.ptr(x)
    assert fill(2, -1, 2, F64, F64, px, px, px, px, px) != 0 and "negative dimension" in err()
    assert fill(2, 2, 1, F64, F64, px, px, px, px, px) != 0 and "ld 1 is smaller" in err()
    assert fill(2, 2, 2, 9, F64, px, px, px, px, px) != 0 and "unsupported dense dtype" in err()
    assert fill(2, 2, 2, F64, F32, px, px, px, px, px) != 0 and "unsupported output dtype" in err()
    assert fill(2, 2, 2, F64, F64, px, px, px, px, None) != 0 and "null pointer" in err()
    assert fill(2, 2, 2, F64, F64, None, px, px, px, px) != 0 and "null pointer" in err()
    scatter = lambda nseg, nother, vd, ld, odt, *ptrs: lib.mxd_csr_to_dense(nseg, nother, ptrs[0], px, px, vd, 0, 0, ptrs[1],  # noqa: E731
                                                                         ld, odt, ptrs[2], None)
    assert scatter(-1, 2, F64, 2, F64, px, px, px) != 0 and "negative dimension" in err()
    assert scatter(2, 2, F64, 1, F64, px, px, px) != 0 and "ld 1 is smaller" in err()
    assert scatter(2, 2, I32, 2, F64, px, px, px) != 0 and "unsupported value dtype" in err()
    assert scatter(2, 2, F64, 2, F32, px, px, px) != 0 and "unsupported output dtype" in err()
    assert scatter(2, 2, F64, 2, F64, None, px, px) != 0 and "null pointer" in err()
    assert scatter(2, 2, F64, 2, F64, px, None, px) != 0 and "null pointer" in err()
    assert scatter(2, 2, F64, 2, F64, px, px, None) != 0 and "null pointer" in err()
    assert lib.mxd_dense_to_csr_workspace_bytes(-1, 2, 0, 0) == 0 and lib.mxd_dense_to_csr_workspace_bytes(2, 2, 0, -1) == 0
    # the export level
    res, info = C.c_void_p(), _lib.ResultInfo()
    begin = lambda *a: lib.mx_dense_to_csr_begin(*a, C.byref(res), C.byref(info))       # noqa: E731
    assert lib.mx_dense_to_csr_begin(px, 2, 2, F64, 0, F64, None, None) != 0 and "null pointer" in err()
    assert begin(px, -2, 2, F64, 0, F64) != 0 and "negative dimension" in err()
    assert begin(px, 2, 2, NONE, 0, F64) != 0 and "unsupported dense dtype" in err()
    assert begin(px, 2, 2, F64, 0, F32) != 0 and "unsupported output dtype" in err()
    assert begin(None, 2, 2, F64, 0, F64) != 0 and "null pointer" in err()
    assert res.value is None
    p = np.zeros(3, np.int32)
    one = np.array([0, 1, 1], np.int32)
    dense = lambda ip, nseg, nother, j, v, vd, out, odt: lib.mx_csr_to_dense(_lib.ptr(ip), nseg, nother, j, v, vd, 0, out, odt)  # noqa: E731
    assert dense(p, -2, 2, None, None, F64, px, F64) != 0 and "negative dimension" in err()
    assert dense(p, 2, 2, None, None, F32, px, F64) != 0 and "unsupported value dtype" in err()
    assert dense(p, 2, 2, None, None, F64, px, F32) != 0 and "unsupported output dtype" in err()
    assert dense(p, 2, 2, None, None, F64, None, F64) != 0 and "null pointer" in err()
    assert dense(one, 2, 2, None, None, NONE, px, F64) != 0 and "null pointer" in err()          # entries, no indices
    assert dense(one, 2, 2, _lib.ptr(p), None, F64, px, F64) != 0 and "null pointer" in err()    # no values
    assert dense(np.array([0, 1, -1], np.int32), 2, 2, None, None, F64, px, F64) != 0 and "bad index pointer" in err()
    assert lib.mx_csr_to_dense(None, 2, 2, None, None, F64, 0, px, F64) != 0 and "null pointer" in err()
    with pytest.raises(ValueError, match="2-d"):
        G.dense_to_csr(np.zeros(3))
    with pytest.raises(TypeError, match="float64, float32, int32 or bool"):
        G.dense_to_csr(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match="out_dtype"):
        G.dense_to_csr(np.zeros((2, 2)), False, F32)
    with pytest.raises(ValueError, match="do not form a CSR"):
        G.csr_to_dense(one, np.zeros(0, np.int32), None, 2)


# ---- device.py on the recording fake ---------------------------------------------------------------------------------
def run(operands, fn, script=None):
    return T.run_case(dict(operands=lambda: operands, run=fn, script=script or {}))


def test_device_dense_to_csr_makes_the_two_calls():
    X = torch.ones((4, 3), dtype=torch.float64).t()                      # 3 x 4, column-major: strides (1, 3)
    out = run(dict(X=X), lambda o: D.dense_to_csr(o["X"]), {"mxd_dense_to_csr_count": [[5]]})
    ws = T.workspace_bytes(3, 4, 0, 0)
    head = [3, 4, ["X", 0], 3, F64, 0, 0, ["fresh#1", 0], ["fresh#0", 0]]
    assert out["calls"] == [
        {"fn": "mxd_dense_to_csr_workspace_bytes", "args": [3, 4, 0, 0]},
        {"fn": "mxd_dense_to_csr_count", "args": head + [["cell", "int64"], "stream"]},
        {"fn": "mxd_dense_to_csr_fill", "args": head + [["fresh#2", 0], ["fresh#3", 0], F64, "stream"]}]
    assert out["allocations"] == [{"dtype": "torch.uint8", "shape": [ws]}, {"dtype": "torch.int32", "shape": [4]},
                                  {"dtype": "torch.int32", "shape": [5]}, {"dtype": "torch.float64", "shape": [5]}]
    r = out["returns"]["DeviceCSR"]
    assert (r["m"], r["K"], r["nnz"]) == (3, 4, 5) and r["indptr"]["storage"] == ["fresh#1", 0]


def test_device_dense_to_csr_reads_strided_operands_in_place():
    big = torch.ones((3, 6), dtype=torch.float32)
    # row-major with a leading dimension of 6: read as the column-major 4 x 3 transpose, so the CSR is its CSC
    out = run(dict(big=big), lambda o: D.dense_to_csr(o["big"][:, :4], out_kind=NONE), {"mxd_dense_to_csr_count": [[0]]})
    assert out["calls"][0] == {"fn": "mxd_dense_to_csr_workspace_bytes", "args": [4, 3, 1, 0]}
    assert out["calls"][1]["args"][:7] == [4, 3, ["big", 0], 6, F32, 1, 0]
    assert [c["fn"] for c in out["calls"]] == ["mxd_dense_to_csr_workspace_bytes", "mxd_dense_to_csr_count"]   # empty: no fill
    r = out["returns"]["DeviceCSR"]
    assert (r["m"], r["K"], r["nnz"]) == (3, 4, 0) and r["values"] == {"value": None}
    # a column-major window of a taller matrix, by_col, logical output, int32 read as R logicals; col_splits passed on
    tall = torch.ones((4, 7), dtype=torch.int32).t()                    # 7 x 4 column-major
    out = run(dict(tall=tall), lambda o: D.dense_to_csr(o["tall"][2:5, 1:], by_col=True, out_kind=LGL, logical=True,
                                                        col_splits=3), {"mxd_dense_to_csr_count": [[2]]})
    assert out["calls"][0]["args"] == [3, 3, 1, 3]
    assert out["calls"][1]["args"][:7] == [3, 3, ["tall", 4 * (7 + 2)], 7, LGL, 1, 3]
    assert out["calls"][2]["args"][-2] == LGL
    r = out["returns"]["DeviceCSR"]
    assert (r["m"], r["K"], r["nnz"]) == (3, 3, 2) and r["values"]["tensor"] == "torch.int32"
    # bool becomes int32 R logicals in a copy; an int32 without `logical` is an R integer
    out = run(dict(b=torch.ones((2, 2), dtype=torch.bool)), lambda o: D.dense_to_csr(o["b"]), {"mxd_dense_to_csr_count": [[4]]})
    assert out["calls"][1]["args"][2] == "other" and out["calls"][1]["args"][4] == LGL
    out = run(dict(i=torch.ones((2, 2), dtype=torch.int32)), lambda o: D.dense_to_csr(o["i"]), {"mxd_dense_to_csr_count": [[4]]})
    assert out["calls"][1]["args"][4] == I32


def test_device_csr_to_dense_makes_one_call():
    out = run(dict(A=T.csr("l")), lambda o: D.csr_to_dense(o["A"]))
    assert out["calls"] == [{"fn": "mxd_csr_to_dense", "args": [3, 4, ["A.indptr", 0], ["A.indices", 0], ["A.values", 0], LGL, 0,
                                                                 0, ["fresh#0", 0], 3, F64, ["fresh#1", 0], "stream"]}]
    assert out["allocations"] == [{"dtype": "torch.float64", "shape": [4, 3]}, {"dtype": "torch.int32", "shape": [1]}]
    r = out["returns"]
    assert r["shape"] == [3, 4] and r["strides"] == [1, 3] and r["storage"] == ["fresh#0", 0]
    # by_col: A holds the CSC arrays of a 4 x 3 matrix; a row-major `out` with padding flips by_col again
    target = torch.zeros((4, 5), dtype=torch.int32)
    flag = torch.zeros(1, dtype=torch.int32)
    out = run(dict(A=T.csr("n"), target=target, flag=flag),
              lambda o: D.csr_to_dense(o["A"], by_col=True, out=o["target"][:, :3], logical=True, flag=o["flag"], col_splits=2))
    assert out["calls"] == [{"fn": "mxd_csr_to_dense", "args": [3, 4, ["A.indptr", 0], ["A.indices", 0], "null", NONE, 0, 2,
                                                                 ["target", 0], 5, LGL, ["flag", 0], "stream"]}]
    assert out["allocations"] == []


def test_device_wrappers_refuse_what_they_cannot_read():
    def refusal(fn):
        return T.run_refusal(dict(operands=lambda: dict(A=T.csr()), run=fn))
    assert refusal(lambda o: D.dense_to_csr(torch.ones(3)))["message"] == "dense_to_csr: the dense operand must be 2-d, got 1-d"
    assert refusal(lambda o: D.dense_to_csr(torch.ones(3, 3), out_kind=F32))["type"] == "ValueError"
    assert refusal(lambda o: D.dense_to_csr(torch.ones(3, 3, dtype=torch.int64)))["message"].startswith("dense_to_csr: unsupported")
    assert "out must be a (3, 4)" in refusal(lambda o: D.csr_to_dense(o["A"], out=torch.zeros(4, 3, dtype=torch.float64)))["message"]
    assert "out must be a (3, 4)" in refusal(lambda o: D.csr_to_dense(o["A"], out=torch.zeros(3, 4)))["message"]
    both = torch.zeros(6, 8, dtype=torch.float64)[::2, ::2]
    assert "contiguous rows or contiguous columns" in refusal(lambda o: D.csr_to_dense(o["A"], out=both))["message"]


# ---- the mirror --------------------------------------------------------------------------------------------------------
KIND_OF = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32", np.dtype(np.int32): "i32", np.dtype(np.bool_): "lgl"}
OUT_OF = {F64: "d", LGL: "l", NONE: "n"}


@pytest.fixture
def calls(monkeypatch):
    """exports.dense_to_csr / csr_to_dense record their arguments and answer from the model; the other exports the
    conversions go through answer in numpy"""
    seen = []

    def dense_to_csr(dense, by_col=False, out_dtype=F64):
        M = np.asarray(dense)
        seen.append(("dense_to_csr", M.dtype, bool(by_col), out_dtype))
        kind = KIND_OF[M.dtype]
        p, j, x = DM.dense_to_csr(M.astype(np.int32) if kind == "lgl" else M, kind, by_col, OUT_OF[out_dtype])
        return dict(indptr=p, indices=j, values=x)

    def csr_to_dense(indptr, indices, values, nother, by_col=False, logical=False):
        seen.append(("csr_to_dense", None if values is None else values.dtype, bool(by_col), bool(logical)))
        return DM.csr_to_dense(indptr, indices, values, nother, by_col, logical)

    def coo_to_csr(i, j, values, nrow, ncol):                           # distinct cells only: nothing to merge
        order = np.lexsort((j, i))
        p = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nrow))]).astype(np.int32)
        return dict(indptr=p, indices=j[order], values=None if values is None else values[order])

    monkeypatch.setattr(G, "dense_to_csr", dense_to_csr)
    monkeypatch.setattr(G, "csr_to_dense", csr_to_dense)
    monkeypatch.setattr(G, "coo_to_csr", coo_to_csr)
    monkeypatch.setattr(G, "csr_to_coo", lambda p: np.repeat(np.arange(p.size - 1, dtype=np.int32), np.diff(p)))
    return seen


@pytest.fixture
def route():
    options["mxgpu.dense_route"] = True
    yield
    options.pop("mxgpu.dense_route", None)


def dense_case():
    M = np.array([[0.0, 2.0, 0.0, -0.0], [np.nan, 0.0, 3.5, 0.0], [0.0, 0.0, 0.0, 0.0]])
    return M, [["a", "b", "c"], ["w", "x", "y", "z"]]


def test_with_the_option_off_nothing_new_is_reached(calls):
    M, names = dense_case()
    assert not options.get("mxgpu.dense_route", False)
    R = mx.as_csr_matrix(mx.DenseMatrix(M, names))
    assert type(R) is mx.dgRMatrix and R.Dimnames == names and R.p.tolist() == [0, 1, 3, 3] and R.j.tolist() == [1, 0, 2]
    assert R.toarray().shape == (3, 4) and np.array_equal(np.isnan(R.toarray()), np.isnan(M))
    T_ =mx.dgTMatrix([2, 0], [1, 3], [1.0, 2.0], (3, 4))
    assert T_.toarray()[2, 1] == 1.0
    # today's host route: a NaN cell is TRUE under logical=TRUE and NA_integer_ is read as a number
    assert mx.as_csr_matrix(M, logical=True).x.tolist() == [1, 1, 1]
    assert mx.as_csr_matrix(np.array([[NA, 0]], np.int32)).x.tolist() == [-2147483648.0]
    assert [c for c in calls if c[0] in ("dense_to_csr", "csr_to_dense")] == []


INPUTS = {
    "ndarray": lambda M, names: (M, [None, None], np.float64),
    "DenseMatrix": lambda M, names: (mx.DenseMatrix(M, names), names, np.float64),
    "float32": lambda M, names: (mx.float32(M, names), names, np.float32),
    "int32": lambda M, names: (np.nan_to_num(M).astype(np.int32), [None, None], np.int32),
    "bool": lambda M, names: (np.nan_to_num(M) != 0, [None, None], np.bool_),
}


@pytest.mark.parametrize("which", list(INPUTS))
def test_with_the_option_on_every_input_type_takes_the_device_route(calls, route, which):
    M, names = dense_case()
    x, want_names, dtype = INPUTS[which](M, names)
    data = x.Data if which == "float32" else np.asarray(x)
    kind = KIND_OF[np.dtype(dtype)]
    as_int = data.astype(np.int32) if kind == "lgl" else data
    for kw, cls, out, code in ((dict(), mx.dgRMatrix, "d", F64), (dict(logical=True), mx.lgRMatrix, "l", LGL),
                               (dict(binary=True), mx.ngRMatrix, "n", NONE)):
        del calls[:]
        R = mx.as_csr_matrix(x, **kw)
        assert calls == [("dense_to_csr", np.dtype(dtype), False, code)]
        p, j, v = DM.dense_to_csr(as_int, kind, False, out)
        assert type(R) is cls and R.Dim == (3, 4) and R.Dimnames == want_names
        assert np.array_equal(R.p, p) and np.array_equal(R.j, j) and np.array_equal(bits(R.x), bits(v))
    del calls[:]
    Cc = mx.as_csc_matrix(x)
    assert calls == [("dense_to_csr", np.dtype(dtype), True, F64)]
    p, i, v = DM.dense_to_csr(as_int, kind, True, "d")
    assert type(Cc) is mx.dgCMatrix and Cc.Dim == (3, 4) and Cc.Dimnames == want_names
    assert np.array_equal(Cc.p, p) and np.array_equal(Cc.i, i) and np.array_equal(bits(Cc.x), bits(v))
    del calls[:]
    Tt = mx.as_coo_matrix(x)                                             # through the CSR: the triplets in row-major order
    assert calls == [("dense_to_csr", np.dtype(dtype), False, F64)]
    p, j, v = DM.dense_to_csr(as_int, kind, False, "d")
    assert type(Tt) is mx.dgTMatrix and Tt.Dim == (3, 4) and Tt.Dimnames == want_names
    assert np.array_equal(Tt.i, np.repeat(np.arange(3), np.diff(p))) and np.array_equal(Tt.j, j)
    assert np.array_equal(bits(Tt.x), bits(v))
    assert type(mx.as_coo_matrix(x, binary=True)) is mx.ngTMatrix and type(mx.as_coo_matrix(x, logical=True)) is mx.lgTMatrix


def test_the_two_corrected_cases(calls, route):
    R = mx.as_csr_matrix(np.array([[NA, 0], [0, 7]], np.int32))
    assert type(R) is mx.dgRMatrix and bits(R.x).tolist() == [0x7FF00000000007A2, bits(np.array([7.0]))[0]]   # NA_real_
    M, _ = dense_case()
    L = mx.as_csr_matrix(M, logical=True)
    assert type(L) is mx.lgRMatrix and L.j.tolist() == [1, 0, 2] and L.x.tolist() == [1, NA, 1]                # NaN -> NA
    assert mx.as_coo_matrix(M, logical=True).x.tolist() == [1, NA, 1]
    assert mx.as_csr_matrix(np.array([[True, False]])).x.tolist() == [1.0]


def test_a_vector_and_a_sparse_input_stay_where_they_were(calls, route):
    R = mx.dgRMatrix([0, 1, 2], [1, 0], [1.0, 2.0], (2, 2))
    assert mx.as_csr_matrix(R) is R
    assert [c for c in calls if c[0] == "dense_to_csr"] == []


def test_as_matrix_and_toarray_under_the_option(calls, route):
    names = [["a", "b"], ["x", "y", "z"]]
    R = mx.dgRMatrix([0, 1, 3], [2, 0, 1], [1.5, np.nan, -2.0], (2, 3), names)
    want = np.array([[0.0, 0.0, 1.5], [np.nan, -2.0, 0.0]])
    out = mx.as_matrix(R)
    assert type(out) is mx.DenseMatrix and out.Dimnames == names and out.flags.f_contiguous
    np.testing.assert_array_equal(np.asarray(out), want)
    assert calls[-1] == ("csr_to_dense", np.dtype(np.float64), False, False)
    np.testing.assert_array_equal(R.toarray(), want)
    assert type(R.toarray()) is np.ndarray and calls[-1][0] == "csr_to_dense"
    Cc = mx.dgCMatrix([0, 1, 1, 2], [1, 0], [4.0, 5.0], (2, 3), names)
    np.testing.assert_array_equal(np.asarray(mx.as_matrix(Cc)), np.array([[0.0, 0.0, 5.0], [4.0, 0.0, 0.0]]))
    assert calls[-1] == ("csr_to_dense", np.dtype(np.float64), True, False)
    Lg = mx.lgRMatrix([0, 2, 2], [0, 2], [NA, 1], (2, 3))
    assert np.asarray(mx.as_matrix(Lg, logical=True)).tolist() == [[NA, 0, 1], [0, 0, 0]]
    assert bits(np.asarray(mx.as_matrix(Lg)))[0, 0] == 0x7FF00000000007A2 and calls[-1][1] == np.dtype(np.int32)
    N = mx.ngRMatrix([0, 1, 1], [1], None, (2, 3))
    assert np.asarray(mx.as_matrix(N)).tolist() == [[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]] and calls[-1][1] is None
    Tt = mx.dgTMatrix([1, 0], [0, 2], [7.0, 8.0], (2, 3), names)
    out = mx.as_matrix(Tt)                                               # through coo_to_csr first
    assert out.Dimnames == names and np.asarray(out).tolist() == [[0.0, 0.0, 8.0], [7.0, 0.0, 0.0]]
    np.testing.assert_array_equal(Tt.toarray(), np.asarray(out))
    with pytest.raises(mx.MatrixExtraError, match="as_matrix: unsupported class"):
        mx.as_matrix(np.zeros((2, 2)))


def test_as_matrix_expands_a_structured_operand_first(calls, route, monkeypatch):
    S = np.array([[1.0, 2.0], [2.0, 0.0]])

    def symmetric_to_general(indptr, indices, values, uplo, value_dtype=None):
        p, j, x = DM.dense_to_csr(S, "f64", False, "d")
        return dict(indptr=p, indices=j, values=x)
    monkeypatch.setattr(G, "csr_symmetric_to_general", symmetric_to_general)
    monkeypatch.setattr(G, "csr_triangle_check", lambda p, j, uplo, strict=False: 0)
    Sy = mx.dsRMatrix([0, 2, 2], [0, 1], [1.0, 2.0], (2, 2), uplo="U")
    assert np.asarray(mx.as_matrix(Sy)).tolist() == S.tolist()
    assert Sy.toarray().tolist() == S.tolist() and calls[-1][0] == "csr_to_dense"
