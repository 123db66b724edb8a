"""The transposed products on device-resident operands (matrixextra_amd/device.py: DeviceCSR.entry_rows / transposed,
spmv_t, spmm_t).  spmv_t must be, bit for bit, col_reduce of the written-out product through the same order; spmm_t must
be spmm on the arrays mxd_csr_transpose returns, the same kernel on identical arrays; both are compared with dense
numpy at the tolerances of tests/test_gpu_host_mirror.py; and the column order is built once however often they run."""
import numpy as np
import pytest

from conftest import csr_to_dense, rand_csr
from devmem import dev_csr_transpose

pytestmark = pytest.mark.gpu

M, K = 300, 70


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64 if t.element_size() == 8 else np.uint32)


@pytest.fixture(scope="module")
def operand(gpu):
    from matrixextra_amd import device as dv
    p, j, x = rand_csr(M, K, 0.2, 41, sorted_cols=False)
    return dv.DeviceCSR.from_host(p, j, x, K), (p, j, x), csr_to_dense(p, j, x, K)


def test_spmv_t_is_col_reduce_of_the_written_out_product(operand):
    import torch
    from matrixextra_amd import device as dv
    A, (p, j, x), D = operand
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(p))).cuda()
    for seed in (1, 2, 3):
        v = torch.from_numpy(np.random.default_rng(seed).normal(size=M)).cuda()
        got = dv.spmv_t(A, v)
        Y = dv.DeviceCSR(A.indptr, A.indices, A.values * v[rows], M, K, A.nnz)         # torch's product: rounded once
        want = dv.col_reduce(Y, "sum", order=A.column_order())
        assert got.dtype == torch.float64 and tuple(got.shape) == (K,)
        assert np.array_equal(bits(got), bits(want))
        assert np.allclose(got.cpu().numpy(), D.T @ v.cpu().numpy(), rtol=1e-10, atol=1e-12)
        assert np.array_equal(bits(dv.spmv_t(A, v)), bits(got))                         # a repeated call: the same bits
        out = torch.full((K,), 7.0, dtype=torch.float64, device="cuda")
        assert dv.spmv_t(A, v, out=out) is out and np.array_equal(bits(out), bits(got))
        # a matrix that shares the pattern uses A's order and builds none of its own
        B = dv.DeviceCSR(A.indptr, A.indices, A.values * 2.0, M, K, A.nnz)
        assert np.array_equal(bits(dv.spmv_t(B, v, order=A.column_order())), bits(got * 2.0))
        assert B._order is None and B._order_builds == 0
    T = A.transposed()
    assert A._order_builds == 1 and T._sorted is True and (T.m, T.K, T.nnz) == (K, M, A.nnz)
    assert T.indptr is A.column_order()[1] and T.indices is A.entry_rows()
    with pytest.raises(ValueError, match="v must have 300 elements"):
        dv.spmv_t(A, torch.zeros(K, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="the order belongs to another pattern"):
        dv.spmv_t(A, torch.zeros(M, dtype=torch.float64, device="cuda"), order=(A.column_order()[0][:-1], A.column_order()[1]))


def test_spmv_t_of_a_pattern_counts_the_rows(operand):
    import torch
    from matrixextra_amd import device as dv
    A, (p, j, x), D = operand
    P = dv.DeviceCSR(A.indptr, A.indices, None, M, K, A.nnz)
    v = torch.from_numpy(np.random.default_rng(4).integers(-9, 10, size=M).astype(np.float64)).cuda()
    got = dv.spmv_t(P, v).cpu().numpy()
    assert np.array_equal(got, (D != 0).T.astype(np.float64) @ v.cpu().numpy())
    assert P.transposed().values is None


@pytest.mark.parametrize("colmajor", [False, True], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [1, 5, 64])
def test_spmm_t(operand, n, dtype, colmajor):
    import torch
    from matrixextra_amd import device as dv
    A, (p, j, x), D = operand
    B = np.random.default_rng(n).normal(size=(M, n)).astype(dtype)
    dB = torch.from_numpy(B).cuda()
    got = dv.spmm_t(A, dB, colmajor=colmajor)
    assert tuple(got.shape) == (K, n) and got.dtype == dB.dtype
    tp, tj, tx = dev_csr_transpose(p, j, x, K)
    T = dv.DeviceCSR.from_host(tp, tj, tx, M)
    want = dv.spmm(T, dB, colmajor=colmajor)
    assert np.array_equal(bits(got.contiguous()), bits(want.contiguous()))
    ref = D.T @ B.astype(np.float64)
    if dtype == "float64":
        assert np.allclose(got.cpu().numpy(), ref, rtol=1e-10, atol=1e-12)
    else:
        assert np.allclose(got.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    out = torch.empty((n, K) if colmajor else (K, n), dtype=dB.dtype, device="cuda")
    res = dv.spmm_t(A, dB, out=out, colmajor=colmajor)
    assert res.data_ptr() == out.data_ptr() and np.array_equal(bits(res.contiguous()), bits(got.contiguous()))
    assert A._order_builds == 1


def test_an_empty_matrix(gpu):
    import torch
    from matrixextra_amd import device as dv
    E = dv.DeviceCSR.from_host(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0), 4)
    v = torch.ones(5, dtype=torch.float64, device="cuda")
    assert np.array_equal(dv.spmv_t(E, v).cpu().numpy(), np.zeros(4))
    T = E.transposed()
    assert (T.m, T.K, T.nnz) == (4, 5, 0) and np.array_equal(T.indptr.cpu().numpy(), np.zeros(5, np.int32))
    for colmajor in (False, True):
        got = dv.spmm_t(E, torch.ones((5, 3), dtype=torch.float64, device="cuda"), colmajor=colmajor)
        assert tuple(got.shape) == (4, 3) and not got.cpu().numpy().any()
    assert E._order_builds == 1
