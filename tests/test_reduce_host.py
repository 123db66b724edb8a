"""The reduction family without a GPU: the CPU model (tests/reduce_model.py) against dense numpy, the mirror's
argument checks and messages, the divisors of the means, norm's type table, and the C-ABI of include/mxgpu_reduce.h
(parsed, exported, bound with its prototypes' types) beside an untouched include/mxgpu.h."""
import ctypes as C
import hashlib
import math
import os

import numpy as np
import pytest

import matrixextra_amd as mx
import reduce_model as RM
from conftest import csr_to_dense, rand_csr
from matrixextra_amd import _lib, reduce as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 70, 0.2), (50, 80, 0.1), (80, 50, 0.1), (1, 1, 1.0), (7, 1, 0.5), (3, 257, 0.05), (0, 4, 0.5), (4, 0, 0.5)]


def shape_id(s):
    return "%dx%d" % s[:2]


# ---- the model against dense numpy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("sorted_cols", [True, False], ids=["sorted", "unsorted"])
def test_model_margins_match_dense_numpy(shape, sorted_cols):
    m, n, dens = shape
    p, j, x = rand_csr(m, n, dens, seed=m * 1000 + n, sorted_cols=sorted_cols)
    D = csr_to_dense(p, j, x, n)
    for op, dense_op in ((RM.SUM, lambda A: A), (RM.ABS_SUM, np.abs), (RM.SQ_SUM, np.square)):
        for over_rows in (True, False):
            got, skipped, bnd = RM.margin(op, p, j, x, "d", m, n, over_rows)
            want = dense_op(D).sum(axis=1 if over_rows else 0)
            assert got.shape == want.shape and not skipped.any()
            # numpy's pairwise sum over the n (or m) cells of a dense row obeys the same any-order bound
            slack = RM.gamma(max(m, n, 1) + 2) * dense_op(np.abs(D)).sum(axis=1 if over_rows else 0)
            assert np.all(np.abs(got - want) <= bnd + slack)
    for over_rows in (True, False):
        got = RM.margin(RM.ABS_MAX, p, j, x, "d", m, n, over_rows)[0]
        want = np.abs(D).max(axis=1 if over_rows else 0) if m and n else np.zeros(m if over_rows else n)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_model_column_order_diag_and_norm_match_dense_numpy(shape):
    m, n, dens = shape
    p, j, x = rand_csr(m, n, dens, seed=m * 1000 + n + 1, sorted_cols=False)
    D = csr_to_dense(p, j, x, n)
    perm, colptr = RM.column_order(j, n)
    rows = np.repeat(np.arange(m), np.diff(p))
    assert np.array_equal(perm, np.lexsort((np.arange(j.size), j)))
    assert np.all(np.diff(j[perm]) >= 0) and np.array_equal(colptr, np.searchsorted(j[perm], np.arange(n + 1)))
    same_col = np.diff(j[perm]) == 0
    assert np.all(np.diff(rows[perm])[same_col] >= 0)                   # stable: rows ascend inside a column
    assert np.array_equal(RM.diag(p, j, x, "d", m, n), np.diag(D)[:min(m, n)] if m and n else np.zeros(0))
    if m and n and j.size:
        want = {"O": np.linalg.norm(D, 1), "I": np.linalg.norm(D, np.inf), "F": np.linalg.norm(D, "fro"),
                "M": np.abs(D).max()}
        for t, kind in RM.NORM_KINDS.items():
            got, bnd = RM.norm(p, j, x, "d", m, n, t)
            assert abs(got - want[kind]) <= bnd + 1e-13 * want[kind], (t, got, want[kind])
    else:
        assert all(RM.norm(p, j, x, "d", m, n, t) == (0.0, 0.0) for t in RM.NORM_KINDS)


def test_model_exact_data_equals_numpy_whatever_the_order():
    for name, segptr in RM.segment_cases().items():
        nnz = int(segptr[-1])
        v, _ = RM.case_values(name, nnz, "exact")
        perm = np.random.default_rng(3).permutation(nnz)
        for op in (RM.SUM, RM.ABS_SUM, RM.SQ_SUM):
            out = RM.segment_reduce(op, v, segptr, perm)[0]
            t = RM._map(op, v[perm])
            want = np.array([t[segptr[s]:segptr[s + 1]].sum() for s in range(segptr.size - 1)])
            assert np.array_equal(out, want), name


def test_model_na_rules():
    f = RM.as_f64(np.array([1, 0, RM.NA_LOGICAL, 5], dtype=np.int32), "l", 4)
    assert np.array_equal(np.isnan(f), [False, False, True, False]) and np.array_equal(f[[0, 1, 3]], [1.0, 0.0, 1.0])
    assert np.array_equal(RM.as_f64(None, "n", 3), np.ones(3))
    seg = np.array([0, 2, 4, 4])
    for op in RM.OPS:
        out, skipped, _ = RM.segment_reduce(op, f, seg)
        assert not np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 0.0 and not skipped.any()
        out, skipped, _ = RM.segment_reduce(op, f, seg, na_rm=True)
        assert np.array_equal(out, [1.0, 1.0, 0.0]) and np.array_equal(skipped, [0, 1, 0])
    x = np.array([3.0, np.nan, -7.0, np.inf, -0.0])
    assert np.isnan(RM.segment_reduce(RM.ABS_MAX, x, [0, 5])[0][0])     # a NaN inside the segment surfaces
    assert RM.segment_reduce(RM.ABS_MAX, x, [0, 5], na_rm=True)[0][0] == np.inf
    assert RM.segment_reduce(RM.ABS_MAX, x, [0, 3], na_rm=True)[0][0] == 7.0
    assert np.isnan(RM.segment_reduce(RM.SUM, np.array([np.inf, -np.inf]), [0, 2])[0][0])


def test_model_means_divide_by_the_cells_less_the_skipped_nas():
    # 3 x 4: row 0 = (2, NA, ., .), row 1 = all four cells stored NAs, row 2 empty
    p, j = np.array([0, 2, 6, 6], dtype=np.int32), np.array([0, 1, 0, 1, 2, 3], dtype=np.int32)
    x = np.array([2.0, np.nan, np.nan, np.nan, np.nan, np.nan])
    out = RM.margin(RM.SUM, p, j, x, "d", 3, 4, True, na_rm=False, mean=True)[0]
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 0.0
    out, skipped, _ = RM.margin(RM.SUM, p, j, x, "d", 3, 4, True, na_rm=True, mean=True)
    assert np.array_equal(skipped, [1, 4, 0])
    assert out[0] == 2.0 / 3.0 and np.isnan(out[1]) and out[2] == 0.0     # 4 - 1 cells; 0 / 0; 0 / 4
    out, skipped, _ = RM.margin(RM.SUM, p, j, x, "d", 3, 4, False, na_rm=True, mean=True)
    assert np.array_equal(skipped, [1, 2, 1, 1])
    assert np.array_equal(out, [2.0 / 2.0, 0.0 / 1.0, 0.0 / 2.0, 0.0 / 2.0])
    out = RM.margin(RM.SUM, p, j, np.arange(1.0, 7.0), "d", 3, 4, False, mean=True)[0]
    assert np.array_equal(out, np.array([1.0 + 3.0, 2.0 + 4.0, 5.0, 6.0]) / 3.0)


# ---- the mirror's checks (nothing here reaches the device) --------------------------------------------------------------
def test_norm_refuses_what_norm_csr_refuses():
    X = mx.dgRMatrix(np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([1.0]), (1, 1))
    for bad in (1, 2.0, None, [], [1], np.array([1])):
        with pytest.raises(mx.MatrixExtraError) as e:
            mx.norm(X, bad)
        assert str(e.value) == "'type' must be a single character variable (see ?norm)."
    for bad in ("E", "", "fro", "OO", ["x", "O"]):
        with pytest.raises(mx.MatrixExtraError) as e:
            mx.norm(X, bad)
        assert str(e.value).startswith("Invalid norm type. Allowed values:")
        assert all(t in str(e.value) for t in R.NORM_TYPES)
    for spectral in ("2", ["2", "O"]):
        with pytest.raises(mx.MatrixExtraError) as e:
            mx.norm(X, spectral)
        assert "spectral norm" in str(e.value) and "Matrix" in str(e.value)


def test_norm_type_table():
    assert R.NORM_TYPES == ("O", "o", "1", "I", "i", "F", "f", "M", "m", "2")
    assert R._NORM_KIND == RM.NORM_KINDS and set(R._NORM_KIND) == set(R.NORM_TYPES) - {"2"}
    assert {R._NORM_KIND[t] for t in "Oo1"} == {"O"} and {R._NORM_KIND[t] for t in "Ii"} == {"I"}
    assert {R._NORM_KIND[t] for t in "Ff"} == {"F"} and {R._NORM_KIND[t] for t in "Mm"} == {"M"}


def test_reductions_refuse_other_operands():
    for fn in (mx.rowSums, mx.colSums, mx.rowMeans, mx.colMeans, mx.diag, mx.norm):
        with pytest.raises(mx.MatrixExtraError):
            fn(np.ones((2, 2)))


def test_mirror_is_exported_and_names_travel():
    for name in ("rowSums", "colSums", "rowMeans", "colMeans", "norm", "diag"):
        assert getattr(mx, name) is getattr(R, name)
    v = R.NamedVector(np.arange(3.0), ["a", "b", "c"])
    assert v.names == ["a", "b", "c"] and isinstance(v, np.ndarray) and v.dtype == np.float64
    assert R.NamedVector(np.arange(2.0)).names is None


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
NEW = ["mx_csr_diag", "mx_csr_margin_reduce", "mx_csr_norm", "mxd_csr_column_order", "mxd_csr_diag", "mxd_segment_reduce"]
P, I, I64, D = C.c_void_p, C.c_int, C.c_int64, C.c_double


def test_reduce_header_parses_and_is_bound_on_the_same_library():
    with open(_lib.REDUCE_HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert sorted(h.functions) == NEW == sorted(_lib.REDUCE_HEADER.functions)
    assert h.constants == {"MX_RED_SUM": 0, "MX_RED_ABS_SUM": 1, "MX_RED_SQ_SUM": 2, "MX_RED_ABS_MAX": 3}
    assert (_lib.MX_RED_SUM, _lib.MX_RED_ABS_SUM, _lib.MX_RED_SQ_SUM, _lib.MX_RED_ABS_MAX) == RM.OPS
    assert h.functions["mxd_segment_reduce"] == (I, (I, P, I, P, I64, P, I, I, P, P, P, P))
    assert h.functions["mxd_csr_column_order"] == (I, (I, I, P, P, I64, P, P, P, P))
    assert h.functions["mxd_csr_diag"] == (I, (I, I, P, P, P, I, I64, I, P, P))
    assert h.functions["mx_csr_margin_reduce"] == (I, (I, I, P, P, P, I, I, I, I, I, P))
    assert h.functions["mx_csr_norm"] == (I, (I, I, P, P, P, I, I, P))
    assert h.functions["mx_csr_diag"] == (I, (I, I, P, P, P, I, P))
    lib = _lib.load()
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)                                         # exported by libmxgpu.so
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name
    with pytest.raises(C.ArgumentError):
        lib.mxd_segment_reduce(0, None, 0, None, 1.5, None, 0, 0, None, None, None, None)


def test_mxgpu_h_is_untouched_and_keeps_its_meaning():
    with open(_lib.HEADER_PATH, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "272d0958dbaeeea098083be2d23248951d00c8726dc60aa6e5f6792e8f5b88b3"
    assert not set(NEW) & set(_lib.declared_symbols()) and not set(NEW) & set(_lib.HEADER.functions)
    assert not any(k.startswith("MX_RED_") for k in _lib.HEADER.constants)


def test_every_prototype_cites_what_it_stands_for():
    with open(_lib.REDUCE_HEADER_PATH) as f:
        text = f.read()
    for name in NEW:
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert "*/" in comment and any(w in comment for w in ("R/csr_linalg.R", "DESIGN.md", "mxd_csr_transpose",
                                                              "rowSums", "mxd_csr_diag")), name


def test_tile_carries_fit_the_published_scratch():
    """a tile carries two f64 partial results and two int32 counts (24 bytes); the header promises that
    4 * mxd_compact_workspace_bytes(nnz) holds them, for one tile of 4096 entries each"""
    lib = _lib.load()
    for nnz in (0, 1, 4095, 4096, 4097, 10 ** 6, 2 ** 31 - 1):
        tiles = -(-nnz // RM.TILE)
        assert 4 * lib.mxd_compact_workspace_bytes(nnz) >= 24 * tiles


def test_calls_fail_loudly_on_bad_arguments():
    lib = _lib.load()
    assert lib.mxd_segment_reduce(7, None, _lib.MX_F64, None, 0, None, 0, 0, None, None, None, None) != 0
    assert "unknown operation" in lib.mx_last_error().decode()
    assert lib.mxd_segment_reduce(0, None, _lib.MX_F32, None, 0, None, 0, 0, None, None, None, None) != 0
    assert "unsupported value dtype" in lib.mx_last_error().decode()
    assert lib.mxd_csr_diag(-1, 2, None, None, None, _lib.MX_F64, 0, 0, None, None) != 0
    assert lib.mxd_csr_column_order(0, 3, None, None, 5, None, None, None, None) != 0
    p = np.array([0, 0], dtype=np.int32)
    out = np.zeros(1)
    assert lib.mx_csr_norm(1, 1, _lib.ptr(p), None, None, _lib.MX_F64, ord("x"), _lib.ptr(out)) != 0
    assert "type must be one of" in lib.mx_last_error().decode()
    assert lib.mx_csr_margin_reduce(1, 1, _lib.ptr(p), None, None, _lib.MX_F64, 2, 0, 0, 0, _lib.ptr(out)) != 0
    assert "axis" in lib.mx_last_error().decode()
    assert math.isfinite(out[0])
