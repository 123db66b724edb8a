"""Device transpose surface checks that need no GPU: the C-ABI entry points exist, t_shallow relabels without
copying, t() follows MatrixExtra.fast_transpose, and t_deep fails loudly without a device."""
import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib


def _small():
    p = np.array([0, 2, 2, 5], dtype=np.int32)
    j = np.array([3, 0, 1, 2, 3], dtype=np.int32)
    x = np.array([1.5, -2.0, 0.0, 4.0, 7.25])
    return mx.dgRMatrix(p, j, x, (3, 4), [["a", "b", "c"], ["w", "x", "y", "z"]])


def test_transpose_entry_points_declared_and_exported():
    names = set(_lib.declared_symbols())
    wanted = {"mx_csr_transpose_begin", "mxd_csr_transpose", "mxd_csr_transpose_workspace_bytes"}
    assert wanted <= names
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in wanted)


def test_transpose_workspace_grows_with_nnz():
    lib = _lib.load()
    small, big = lib.mxd_csr_transpose_workspace_bytes(1000), lib.mxd_csr_transpose_workspace_bytes(1 << 20)
    assert 0 < small < big
    assert big >= 5 * 4 * (1 << 20)          # row ids + two key / payload pairs


def test_t_shallow_relabels_without_copying():
    X = _small()
    T = mx.t_shallow(X)
    assert type(T) is mx.dgCMatrix
    assert T.p is X.p and T.i is X.j and T.x is X.x
    assert T.Dim == (4, 3)
    assert T.Dimnames == [["w", "x", "y", "z"], ["a", "b", "c"]]
    back = mx.t_shallow(T)
    assert type(back) is mx.dgRMatrix
    assert back.p is X.p and back.j is X.j and back.x is X.x
    assert back.Dim == X.Dim and back.Dimnames == X.Dimnames


@pytest.mark.parametrize("cls, missing", [(mx.lgRMatrix, "lgCMatrix"), (mx.ngRMatrix, "ngCMatrix")])
def test_t_shallow_names_the_missing_class(cls, missing):
    X = _small()
    Y = cls(X.p, X.j, None if cls is mx.ngRMatrix else np.ones(X.j.size, dtype=np.int32), X.Dim)
    with pytest.raises(mx.MatrixExtraError, match=missing):
        mx.t_shallow(Y)


def test_fast_transpose_option_defaults_to_deep():
    assert mx.options["MatrixExtra.fast_transpose"] is False


def test_t_with_fast_transpose_gives_a_csc_relabel():
    X = _small()
    old = mx.options["MatrixExtra.fast_transpose"]
    mx.options["MatrixExtra.fast_transpose"] = True
    try:
        T = X.t()
        assert type(T) is mx.dgCMatrix and T.Dim == (4, 3) and T.p is X.p
        assert type(T.t()) is mx.dgRMatrix
    finally:
        mx.options["MatrixExtra.fast_transpose"] = old


@pytest.mark.skipif(_lib.load() is not None and __import__("conftest")._have_gpu(), reason="GPU present")
def test_t_deep_fails_loudly_without_gpu():
    X = _small()
    with pytest.raises(_lib.MxError):
        mx.t_deep(X)
    with pytest.raises(_lib.MxError):
        X.t()
    with pytest.raises(_lib.MxError):
        mx.as_csc_matrix(X)
    with pytest.raises(_lib.MxError):
        mx.as_csr_matrix(mx.t_shallow(X))
