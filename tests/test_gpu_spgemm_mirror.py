"""The sparse x sparse products from the mirror (matrixextra_amd/matmul.py under options["mxgpu.spgemm_route"]), the
export (exports.csr_spgemm) and the resident wrapper (device.spgemm), on the shapes of the reference's operator tests
(tests/testthat/test-operators.R: 100 x 35 at density 0.4, and 35 x 100).  Data is integer-valued, so dense numpy gives
the exact result whatever the order of the sums; the order itself is pinned at device level (tests/test_gpu_spgemm.py)."""
import itertools

import numpy as np
import pytest

import matrixextra_amd as mx
import spgemm_model as SM
from conftest import csr_to_dense, rand_csr
from matrixextra_amd import exports as G
from matrixextra_amd.matrices import options

pytestmark = pytest.mark.gpu
M_, K_ = 100, 35
NA = mx.NA_INTEGER


@pytest.fixture
def route():
    options["mxgpu.spgemm_route"] = True
    yield
    options.pop("mxgpu.spgemm_route", None)


def names(tag, shape):
    return [["%sr%d" % (tag, r) for r in range(shape[0])], ["%sc%d" % (tag, c) for c in range(shape[1])]]


def operand(shape, layout, seed, tag, sorted_cols=True):
    """(matrix, dense) of an integer-valued operand held as CSR ("R") or CSC ("C")"""
    m, n = shape if layout == "R" else shape[::-1]
    p, j, _ = rand_csr(m, n, 0.4, seed, sorted_cols=sorted_cols)
    x = np.random.default_rng(seed).integers(-9, 10, size=j.size).astype(np.float64)
    D = csr_to_dense(p, j, x, n)
    if layout == "R":
        return mx.dgRMatrix(p, j, x, shape, names(tag, shape)), D
    return mx.dgCMatrix(p, j, x, shape, names(tag, shape)), D.T


def dense_of(out):
    if isinstance(out, mx.dgCMatrix):
        return csr_to_dense(out.p, out.i, out.x, out.Dim[0]).T
    return csr_to_dense(out.p, out.j, out.x, out.Dim[1])


SHAPES = {"matmult": ((M_, K_), (K_, M_)), "crossprod": ((M_, K_), (M_, K_)), "tcrossprod": ((M_, K_), (M_, K_))}
CALL = {"matmult": lambda x, y: x @ y, "crossprod": mx.crossprod, "tcrossprod": mx.tcrossprod}
DENSE = {"matmult": lambda X, Y: X @ Y, "crossprod": lambda X, Y: X.T @ Y, "tcrossprod": lambda X, Y: X @ Y.T}


@pytest.mark.parametrize("lx,ly", list(itertools.product("RC", repeat=2)))
@pytest.mark.parametrize("signature", sorted(SHAPES))
def test_every_signature_and_layout_against_dense_numpy(gpu, route, signature, lx, ly):
    sx, sy = SHAPES[signature]
    X, DX = operand(sx, lx, 11, "x", sorted_cols=False)                 # the left-hand operand may be unsorted
    Y, DY = operand(sy, ly, 12, "y")
    out = CALL[signature](X, Y)
    want = DENSE[signature](DX, DY)
    assert type(out) is (mx.dgCMatrix if lx == ly == "C" else mx.dgRMatrix)
    assert out.Dim == want.shape and np.array_equal(dense_of(out), want)
    idx = out.i if isinstance(out, mx.dgCMatrix) else out.j
    assert all(np.all(np.diff(idx[out.p[r]:out.p[r + 1]]) > 0) for r in range(out.p.size - 1))
    assert out.x.dtype == np.float64 and out.p[-1] == idx.size == out.x.size
    rn = X.Dimnames[1] if signature == "crossprod" else X.Dimnames[0]
    cn = Y.Dimnames[0] if signature == "tcrossprod" else Y.Dimnames[1]
    assert out.Dimnames == [rn, cn]
    mx.check_valid_matrix(out)


def test_one_argument_forms_and_an_unsorted_right_hand_operand(gpu, route):
    X, D = operand((M_, K_), "R", 13, "x", sorted_cols=False)
    before = X.j.copy()
    out = mx.crossprod(X)                                               # X is the right-hand operand too: sorted in a copy
    assert type(out) is mx.dgRMatrix and np.array_equal(dense_of(out), D.T @ D) and np.array_equal(X.j, before)
    assert np.array_equal(dense_of(out), dense_of(out).T) and out.Dimnames == [X.Dimnames[1]] * 2
    assert np.array_equal(dense_of(mx.tcrossprod(X)), D @ D.T)
    Cx, Dc = operand((M_, K_), "C", 14, "x")
    out = mx.crossprod(Cx)
    assert type(out) is mx.dgCMatrix and np.array_equal(dense_of(out), Dc.T @ Dc)


def test_logical_pattern_and_structured_operands(gpu, route):
    p, j, xl = rand_csr(M_, K_, 0.4, 15, dtype="l")
    Y, DY = operand((K_, M_), "R", 16, "y")
    assert (xl == NA).any() and (xl == 0).any()
    out = mx.lgRMatrix(p, j, xl, (M_, K_)) @ Y
    want = SM.spgemm(p, j, xl, Y.p, Y.j, Y.x, K_, M_)                   # NA -> NA_real_, a stored FALSE stays an entry
    assert np.array_equal(out.p, want[0]) and np.array_equal(out.j, want[1])
    assert np.array_equal(np.isnan(out.x), np.isnan(want[2])) and np.array_equal(np.nan_to_num(out.x), np.nan_to_num(want[2]))
    assert np.isnan(out.x).any()
    N = mx.ngRMatrix(p, j, None, (M_, K_))
    S = csr_to_dense(p, j, np.ones(j.size), K_)
    assert np.array_equal(dense_of(mx.tcrossprod(N)), S @ S.T) and np.array_equal(dense_of(N @ Y), S @ DY)
    n = K_
    rng = np.random.default_rng(17)
    T = np.triu(np.where(rng.random((n, n)) < 0.4, rng.integers(1, 9, size=(n, n)), 0).astype(np.float64))
    r, c = np.nonzero(T)
    tp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    Sy = mx.dsRMatrix(tp, c, T[r, c], (n, n), uplo="U")
    full = T + T.T - np.diag(np.diag(T))
    assert np.array_equal(dense_of(Sy @ Y), full @ DY) and np.array_equal(dense_of(mx.crossprod(Sy)), full.T @ full)
    Tr = mx.dtRMatrix(tp, c, T[r, c], (n, n), uplo="U", diag="N")
    assert np.array_equal(dense_of(mx.tcrossprod(Tr, Sy)), T @ full.T)


def test_the_export_and_the_resident_wrapper_agree(gpu):
    """exports.csr_spgemm with trans_a against device.spgemm on transposed(): the same arrays, bit for bit, and the
    column order is built once"""
    import torch
    from matrixextra_amd import device as dv
    p, j, x = rand_csr(M_, K_, 0.4, 18, sorted_cols=False)
    x = np.random.default_rng(18).normal(size=j.size)
    q, k, y = rand_csr(M_, K_, 0.4, 19)
    y = np.random.default_rng(19).normal(size=k.size)
    A, Bm = dv.DeviceCSR.from_host(p, j, x, K_), dv.DeviceCSR.from_host(q, k, y, K_)
    for _ in range(2):
        Cd = dv.spgemm(A.transposed(), Bm)                              # crossprod(X, Y) on resident operands
    assert A._order_builds == 1 and Cd._sorted is True and (Cd.m, Cd.K) == (K_, K_)
    res = G.csr_spgemm(p, j, x, (M_, K_), True, q, k, y, (M_, K_), False)
    cp, cj, cx = Cd.to_host()
    assert np.array_equal(cp, res["indptr"]) and np.array_equal(cj, res["indices"])
    assert np.array_equal(cx.view(np.uint64), res["values"].view(np.uint64)) and cx.size == Cd.nnz
    assert np.allclose(csr_to_dense(cp, cj, cx, K_), csr_to_dense(p, j, x, K_).T @ csr_to_dense(q, k, y, K_), rtol=1e-12, atol=1e-12)
    want = SM.spgemm(*[t.cpu().numpy() for t in (A.transposed().indptr, A.transposed().indices, A.transposed().values)],
                     q, k, y, M_, K_)
    assert np.array_equal(cp, want[0]) and np.array_equal(cx.view(np.uint64), want[2].view(np.uint64))
    with pytest.raises(ValueError, match="A has 35 columns, B has 100 rows"):
        dv.spgemm(A, Bm)
    P = dv.DeviceCSR(A.indptr, A.indices, None, M_, K_, A.nnz)           # a pattern on the left, logicals on the right
    Lg = dv.DeviceCSR(Bm.indptr, Bm.indices, torch.ones(Bm.nnz, dtype=torch.int32, device="cuda"), M_, K_, Bm.nnz)
    Cn = dv.spgemm(P.transposed(), Lg)
    S, T = csr_to_dense(p, j, np.ones(j.size), K_), csr_to_dense(q, k, np.ones(k.size), K_)
    assert np.array_equal(csr_to_dense(*Cn.to_host(), K_), S.T @ T)


def test_empty_results(gpu, route):
    z = lambda n: np.zeros(n + 1, np.int32)                             # noqa: E731
    e = np.zeros(0, np.int32)
    p, j, x = rand_csr(6, 4, 0.5, 20)
    for args, shape in (((z(0), e, None, (0, 4), False, p[:5], j[:p[4]], x[:p[4]], (4, 4), False), (0, 4)),
                        ((z(6), e, np.zeros(0), (6, 4), False, z(4), e, np.zeros(0), (4, 9), False), (6, 9)),
                        ((p, j, x, (6, 4), True, z(6), e, None, (6, 3), False), (4, 3)),
                        ((p, j, x, (6, 4), False, z(5), e, None, (5, 4), True), (6, 5))):
        res = G.csr_spgemm(*args)
        assert np.array_equal(res["indptr"], z(shape[0])) and res["indices"].size == 0 and res["values"].size == 0
    E = mx.dgRMatrix(z(6), e, np.zeros(0), (6, 4))
    out = mx.crossprod(E)
    assert out.Dim == (4, 4) and out.p.tolist() == [0] * 5 and out.x.size == 0
