"""The transposed products before a device call: include/mxgpu_tprod.h as the binding reads it, and what the
`%*%` / crossprod / tcrossprod dispatch of matmul.py decides for the signatures that used to end in "Unsupported operand
types": which export each one reaches, with which arrays, and the shape and Dimnames of the result.  The two exports are
replaced by a numpy stand-in, so no GPU is needed."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import matrixextra_amd as mx
from conftest import csr_to_dense, rand_csr
from matrixextra_amd import _lib, exports as G, matmul

NEW = ["mx_csr_tmatmul_dense", "mx_csr_tmatvec", "mxd_csr_transpose_by_order", "mxd_segment_dot"]
P, I, I64 = C.c_void_p, C.c_int, C.c_int64
NA = mx.NA_INTEGER


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_tprod_header_parses_and_is_bound_on_the_same_library():
    with open(_lib.TPROD_HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert sorted(h.functions) == NEW == sorted(_lib.TPROD_HEADER.functions)
    assert h.constants == {} and h.structs == {}
    assert h.functions["mxd_segment_dot"] == (I, (P, I, P, P, P, I64, I64, P, I, P, P, P))
    assert h.functions["mxd_csr_transpose_by_order"] == (I, (I, I64, P, P, I, P, P, P, P))
    assert h.functions["mx_csr_tmatvec"] == (I, (I, I, P, P, P, I, P, P))
    assert h.functions["mx_csr_tmatmul_dense"] == (I, (I, I, P, P, P, P, I, I, I, P, I, I))
    lib = _lib.load()
    for name, (restype, argtypes) in h.functions.items():
        fn = getattr(lib, name)                                         # exported by libmxgpu.so
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name


def test_the_other_headers_keep_their_prototypes():
    assert not set(NEW) & set(_lib.declared_symbols()) and not set(NEW) & set(_lib.HEADER.functions)
    assert _lib.declared_symbols() == sorted(_lib.HEADER.functions)
    assert not set(NEW) & (set(_lib.REDUCE_HEADER.functions) | set(_lib.SYM_HEADER.functions))
    with open(_lib.HEADER_PATH, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "272d0958dbaeeea098083be2d23248951d00c8726dc60aa6e5f6792e8f5b88b3"


def test_every_device_prototype_states_its_synchronisation():
    with open(_lib.TPROD_HEADER_PATH) as f:
        text = f.read()
    for name in ("mxd_segment_dot", "mxd_csr_transpose_by_order"):
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert "no synchronisation" in comment and "One synchronisation" not in comment, name


def test_calls_fail_loudly_on_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.mx_last_error().decode()                          # noqa: E731
    assert lib.mxd_segment_dot(None, _lib.MX_LGL, None, None, None, 0, 0, None, 1, None, None, None) != 0
    assert "unsupported value dtype" in err()
    assert lib.mxd_segment_dot(None, _lib.MX_F64, None, None, None, 0, -1, None, 1, None, None, None) != 0
    assert "bad size" in err()
    assert lib.mxd_segment_dot(None, _lib.MX_F64, None, None, None, 0, 0, None, 1, None, None, None) != 0
    assert "null pointer" in err()
    assert lib.mxd_segment_dot(None, _lib.MX_F64, None, None, None, 0, 0, None, 0, None, None, None) == 0
    assert lib.mxd_csr_transpose_by_order(0, 3, None, None, _lib.MX_NONE, None, None, None, None) != 0
    assert "entries without rows" in err()
    assert lib.mxd_csr_transpose_by_order(2, 3, None, None, _lib.MX_F32, None, None, None, None) != 0
    assert "unsupported value dtype" in err()
    assert lib.mxd_csr_transpose_by_order(2, 0, None, None, _lib.MX_F64, None, None, None, None) == 0
    p = np.zeros(3, np.int32)
    out = np.full(4, 7.0)
    assert lib.mx_csr_tmatvec(2, 4, _lib.ptr(p), None, None, _lib.MX_LGL, None, _lib.ptr(out)) != 0
    assert "unsupported value dtype" in err()
    assert lib.mx_csr_tmatvec(2, 4, None, None, None, _lib.MX_F64, None, _lib.ptr(out)) != 0
    assert "null indptr" in err()
    assert lib.mx_csr_tmatmul_dense(2, 4, _lib.ptr(p), None, None, None, 3, 3, _lib.MX_I32, _lib.ptr(out), 3, 0) != 0
    assert "unsupported dense dtype" in err()
    assert lib.mx_csr_tmatmul_dense(2, 4, _lib.ptr(p), None, None, None, 1, 1, _lib.MX_F64, None, 1, 0) != 0
    assert "null output" in err()


def test_a_matrix_without_entries_gives_zeros_before_any_device_call():
    """the SpMM exports' early-out: no GPU is touched"""
    p = np.zeros(4, np.int32)
    j, x = np.zeros(0, np.int32), np.zeros(0)
    assert np.array_equal(G.csr_tmatvec(p, j, x, 5, np.ones(3)), np.zeros(5))
    assert np.array_equal(G.csr_tmatvec(p, j, None, 5, np.ones(3)), np.zeros(5))
    for dt in (np.float64, np.float32):
        for colmajor in (True, False):
            out = G.csr_tmatmul_dense(p, j, x, 5, np.ones((3, 2), dt), colmajor)
            assert out.shape == (5, 2) and out.dtype == dt and not out.any()
            assert out.flags.f_contiguous if colmajor else out.flags.c_contiguous
    with pytest.raises(ValueError, match="one element per row"):
        G.csr_tmatvec(p, j, x, 5, np.ones(4))
    with pytest.raises(ValueError, match="one row per row"):
        G.csr_tmatmul_dense(p, j, x, 5, np.ones((4, 2)), True)


# ---- the mirror --------------------------------------------------------------------------------------------------------
M_, K_, N_ = 7, 5, 3


def dense_of(p, j, x, K):
    return csr_to_dense(np.asarray(p), np.asarray(j), None if x is None else np.asarray(x), K)


@pytest.fixture
def calls(monkeypatch):
    """the two exports record their arguments and answer in numpy; every other device route fails the test"""
    seen = []

    def tmatvec(indptr, indices, values, ncols, v):
        seen.append(("csr_tmatvec", (indptr, indices, values, ncols, v)))
        assert v.dtype == np.float64 and v.ndim == 1
        with np.errstate(invalid="ignore"):
            S = dense_of(indptr, indices, values, ncols)
            return np.where(S.T != 0, S.T * v[None, :], 0.0).sum(axis=1)    # only stored entries multiply

    def tmatmul(indptr, indices, values, ncols, B, colmajor_out):
        seen.append(("csr_tmatmul_dense", (indptr, indices, values, ncols, B, colmajor_out)))
        assert B.dtype == np.float64 and B.flags.c_contiguous
        with np.errstate(invalid="ignore"):
            out = dense_of(indptr, indices, values, ncols).T @ B
        return np.asfortranarray(out) if colmajor_out else np.ascontiguousarray(out)

    monkeypatch.setattr(G, "csr_tmatvec", tmatvec)
    monkeypatch.setattr(G, "csr_tmatmul_dense", tmatmul)

    def reached(*a, **k):
        raise AssertionError("another device route was reached")
    for name in ("csr_transpose", "tcrossprod_csr_dense_numeric", "matmul_dense_csc_numeric", "matmul_csr_dvec_numeric",
                 "tcrossprod_dense_csr_numeric", "matmul_rowvec_by_csc", "matmul_colvec_by_scolvecascsr"):
        monkeypatch.setattr(G, name, reached)
    return seen


def int_values(n, seed):
    """non-zero integers: every product and sum below is exact, whatever its order"""
    return np.random.default_rng(seed).choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=n)


def csr_X(names=True):
    p, j, _ = rand_csr(M_, K_, 0.5, 3, sorted_cols=False)
    x = int_values(j.size, 30)
    dn = [["r%d" % r for r in range(M_)], ["c%d" % c for c in range(K_)]] if names else None
    return mx.dgRMatrix(p, j, x, (M_, K_), dn), csr_to_dense(p, j, x, K_)


def csc_X(names=True):
    """an M_ x K_ dgCMatrix: its arrays are the CSR of the K_ x M_ transpose"""
    p, i, _ = rand_csr(K_, M_, 0.5, 4, sorted_cols=False)
    x = int_values(i.size, 40)
    dn = [["r%d" % r for r in range(M_)], ["c%d" % c for c in range(K_)]] if names else None
    return mx.dgCMatrix(p, i, x, (M_, K_), dn), csr_to_dense(p, i, x, M_).T


def dense_Y(rows, cols, seed):
    Y = np.random.default_rng(seed).integers(-4, 5, size=(rows, cols)).astype(np.float64)
    return mx.DenseMatrix(Y, [["y%d" % r for r in range(rows)], ["z%d" % c for c in range(cols)]])


def test_crossprod_csr_matrix(calls):
    X, D = csr_X()
    Y = dense_Y(M_, N_, 1)
    out = mx.crossprod(X, Y)
    (name, args), = calls
    assert name == "csr_tmatmul_dense" and args[0] is X.p and args[1] is X.j and args[2] is X.x and args[3] == K_
    assert args[4].shape == (M_, N_) and np.array_equal(args[4], Y) and args[5] is True
    assert isinstance(out, mx.DenseMatrix) and out.shape == (K_, N_) and out.flags.f_contiguous
    assert np.array_equal(out, D.T @ np.asarray(Y))
    assert out.Dimnames == [X.Dimnames[1], Y.Dimnames[1]]


def test_crossprod_csr_vector_and_vector_times_csr(calls):
    X, D = csr_X()
    v = np.arange(1.0, M_ + 1)
    out = mx.crossprod(X, v)
    assert calls[-1][0] == "csr_tmatvec" and calls[-1][1][0] is X.p and calls[-1][1][3] == K_
    assert isinstance(out, mx.DenseMatrix) and out.shape == (K_, 1) and np.array_equal(out[:, 0], D.T @ v)
    assert out.Dimnames == [X.Dimnames[1], None]
    out = v @ X
    assert calls[-1][0] == "csr_tmatvec" and calls[-1][1][1] is X.j and len(calls) == 2
    assert out.shape == (1, K_) and np.array_equal(out[0], v @ D) and out.Dimnames == [None, X.Dimnames[1]]
    assert np.array_equal(matmul.matmul(v, X), out)


def test_matrix_times_csr_hands_over_its_own_buffer(calls):
    X, D = csr_X()
    Y = dense_Y(N_, M_, 2)                                              # N_ x M_, column-major
    out = Y @ X
    (name, args), = calls
    assert name == "csr_tmatmul_dense" and args[0] is X.p and args[3] == K_ and args[5] is False
    B = args[4]
    assert B.shape == (M_, N_) and B.flags.c_contiguous and np.array_equal(B, np.asarray(Y).T)
    assert np.shares_memory(B, Y)                                       # no host transpose: Y's buffer is the row-major t(Y)
    assert isinstance(out, mx.DenseMatrix) and out.shape == (N_, K_) and out.flags.f_contiguous
    assert np.array_equal(out, np.asarray(Y) @ D)
    assert out.Dimnames == [Y.Dimnames[0], X.Dimnames[1]]


def test_csc_times_matrix_and_vector(calls):
    X, D = csc_X()
    Y = dense_Y(K_, N_, 5)
    out = X @ Y
    (name, args), = calls
    assert name == "csr_tmatmul_dense" and args[0] is X.p and args[1] is X.i and args[2] is X.x and args[3] == M_
    assert args[4].shape == (K_, N_) and args[5] is True
    assert out.shape == (M_, N_) and np.array_equal(out, D @ np.asarray(Y))
    assert out.Dimnames == [X.Dimnames[0], Y.Dimnames[1]]
    v = np.arange(1.0, K_ + 1)
    out = X @ v
    assert calls[-1][0] == "csr_tmatvec" and calls[-1][1][1] is X.i and calls[-1][1][3] == M_
    assert out.shape == (M_, 1) and np.array_equal(out[:, 0], D @ v) and out.Dimnames == [X.Dimnames[0], None]


def test_tcrossprod_matrix_csc(calls):
    X, D = csc_X()
    Y = dense_Y(N_, K_, 6)
    out = mx.tcrossprod(Y, X)
    (name, args), = calls
    assert name == "csr_tmatmul_dense" and args[1] is X.i and args[3] == M_ and args[5] is False
    assert args[4].shape == (K_, N_) and np.shares_memory(args[4], Y)
    assert out.shape == (N_, M_) and out.flags.f_contiguous and np.array_equal(out, np.asarray(Y) @ D.T)
    assert out.Dimnames == [Y.Dimnames[0], X.Dimnames[0]]


def test_logical_and_pattern_matrices_become_numeric(calls):
    p, j, xl = rand_csr(M_, K_, 0.5, 7, dtype="l")
    v = np.ones(M_)
    mx.crossprod(mx.lgRMatrix(p, j, xl, (M_, K_)), v)
    x = calls[-1][1][2]
    assert x.dtype == np.float64 and np.array_equal(np.isnan(x), xl == NA) and np.array_equal(x[xl != NA], xl[xl != NA])
    assert (xl == NA).any()
    out = mx.crossprod(mx.ngRMatrix(p, j, None, (M_, K_)), v)
    assert np.array_equal(calls[-1][1][2], np.ones(j.size))
    assert np.array_equal(out[:, 0], np.bincount(j, minlength=K_))


def test_integer_and_logical_dense_operands_become_double_with_na(calls):
    X, D = csr_X()
    vi = np.array([1, NA, 3, 0, -2, NA, 7], dtype=np.int32)
    mx.crossprod(X, vi)
    v = calls[-1][1][4]
    assert v.dtype == np.float64 and np.array_equal(np.isnan(v), vi == NA) and np.array_equal(v[vi != NA], vi[vi != NA])
    assert v[1].view(np.uint64) == np.float64(mx.NA_REAL).view(np.uint64)        # NA_real_, not just any NaN
    matmul.matmul(matmul.RLogical([1, 0, NA, 1, 1, 0, 1]), X)
    assert np.isnan(calls[-1][1][4][2]) and calls[-1][1][4][0] == 1.0
    mx.crossprod(X, np.array([True, False] * 3 + [True]))
    assert calls[-1][1][4].dtype == np.float64 and calls[-1][1][4].sum() == 4.0
    Yi = np.arange(M_ * 2, dtype=np.int32).reshape(M_, 2)
    Yi[3, 1] = NA
    mx.crossprod(X, Yi)
    B = calls[-1][1][4]
    assert B.dtype == np.float64 and np.isnan(B[3, 1]) and np.isnan(B).sum() == 1


def test_dimension_errors(calls):
    X, _ = csr_X()
    C_, _ = csc_X()
    bad_v, bad_m = "Matrix-vector dimensions do not match.", "Matrix dimensions do not match."
    for call in (lambda: mx.crossprod(X, np.ones(M_ + 1)), lambda: np.ones(K_) @ X, lambda: C_ @ np.ones(M_)):
        with pytest.raises(mx.MatrixExtraError, match=bad_v):
            call()
    for call in (lambda: mx.crossprod(X, np.ones((K_, 2))), lambda: np.ones((2, K_)) @ X, lambda: C_ @ np.ones((M_, 2)),
                 lambda: mx.tcrossprod(np.ones((2, M_)), C_)):
        with pytest.raises(mx.MatrixExtraError, match=bad_m):
            call()
    assert calls == []


def test_float32_and_sparse_operands_keep_raising(calls):
    X, _ = csr_X()
    C_, _ = csc_X()
    f_vec, f_mat = mx.float32(np.ones(M_, np.float32)), mx.float32(np.ones((M_, 2), np.float32))
    for call in (lambda: mx.crossprod(X, f_vec), lambda: mx.crossprod(X, f_mat), lambda: mx.crossprod(X, X),
                 lambda: mx.crossprod(f_vec, C_)):
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for crossprod"):
            call()
    for call in (lambda: matmul.matmul(mx.float32(np.ones((2, M_), np.float32)), X), lambda: matmul.matmul(f_vec, X),
                 lambda: matmul.matmul(C_, mx.float32(np.ones((K_, 2), np.float32))),
                 lambda: matmul.matmul(C_, mx.dsparseVector([1], [1.0], K_)), lambda: matmul.matmul(C_, X)):
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for %\\*%"):
            call()
    for call in (lambda: mx.tcrossprod(mx.float32(np.ones((2, K_), np.float32)), C_),
                 lambda: mx.tcrossprod(np.ones(K_), C_)):
        with pytest.raises(mx.MatrixExtraError, match="Unsupported operand types for tcrossprod"):
            call()
    assert calls == []
