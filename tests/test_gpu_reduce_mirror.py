"""The mirror of the reductions on the GPU (matrixextra_amd/reduce.py, the exports behind it and the device-level
wrappers of device.py): rowSums / colSums / rowMeans / colMeans, norm and diag on every operand class, the
export-level calls from host arrays, and the gradient step of the vignette.  Expectations come from
tests/reduce_model.py: exact for integer-valued, logical and pattern data, within the derived any-order bound for
general floats."""
import numpy as np
import pytest

import matrixextra_amd as mx
import reduce_model as RM
from conftest import csr_to_dense, rand_csr
from matrixextra_amd import _lib, exports

pytestmark = pytest.mark.gpu

M, N = 300, 40
ROWN, COLN = ["r%d" % i for i in range(M)], ["c%d" % i for i in range(N)]
MARGINS = [("rowSums", True, False), ("colSums", False, False), ("rowMeans", True, True), ("colMeans", False, True)]


def operand(kind, seed=21):
    """an M x N CSR of the kind with unsorted rows, NAs among its values, an empty row and an empty column"""
    p, j, x = rand_csr(M, N - 1, 0.2, seed, sorted_cols=False, dtype=kind, empty_rows=(17,))
    if kind == "d":
        x = x * 10.0 ** np.random.default_rng(seed).integers(-3, 4, size=x.size)
        x[::37] = np.nan
    cls = {"d": mx.dgRMatrix, "l": mx.lgRMatrix, "n": mx.ngRMatrix}[kind]
    return cls(p, j, x, (M, N), [ROWN, COLN]), (p, j, x)


def check_margins(X, p, j, x, kind, m, n, exact, names):
    for fn, over_rows, mean in MARGINS:
        for na_rm in (False, True):
            got = getattr(mx, fn)(X, na_rm=na_rm)
            want, _, bnd = RM.margin(RM.SUM, p, j, x, kind, m, n, over_rows, na_rm, mean)
            what = f"{fn}(na_rm={na_rm})"
            assert got.dtype == np.float64 and got.names == names[0 if over_rows else 1], what
            RM.assert_reduced(np.asarray(got), None, want, None, np.zeros_like(bnd) if exact and not mean else bnd, what)
            assert np.array_equal(np.asarray(getattr(mx, fn)(X, na_rm=na_rm)).view(np.uint64),
                                  np.asarray(got).view(np.uint64)), f"{what}: a repeated call gave other bits"


@pytest.mark.parametrize("kind", ["d", "l", "n"])
def test_margins_of_a_csr(gpu, kind):
    X, (p, j, x) = operand(kind)
    check_margins(X, p, j, x, kind, M, N, kind != "d", [ROWN, COLN])
    if kind != "n":                                      # the NAs are really there, and na_rm really skips them
        assert np.isnan(np.asarray(mx.rowSums(X))).any() and not np.isnan(np.asarray(mx.rowSums(X, na_rm=True))).any()
    assert mx.rowSums(X)[17] == 0.0 and mx.colMeans(X)[N - 1] == 0.0


def test_margins_of_a_csc(gpu):
    """a dgCMatrix: the same routines with the axes swapped"""
    _, (p, j, x) = operand("d", seed=22)
    Xc = mx.dgCMatrix(p, j, x, (N, M), [COLN, ROWN])     # the CSC slots of the transpose: an N x M matrix
    for fn, over_rows, mean in MARGINS:
        got = getattr(mx, fn)(Xc, na_rm=True)
        want, _, bnd = RM.margin(RM.SUM, p, j, x, "d", M, N, not over_rows, True, mean)
        assert got.names == (COLN if over_rows else ROWN)
        RM.assert_reduced(np.asarray(got), None, want, None, bnd, fn)
    for t in RM.NORM_KINDS:
        swapped = {"O": "I", "I": "O"}.get(RM.NORM_KINDS[t], RM.NORM_KINDS[t])
        clean = np.where(np.isnan(x), 1.0, x)
        want, bnd = RM.norm(p, j, clean, "d", M, N, swapped)
        got = mx.norm(mx.dgCMatrix(p, j, clean, (N, M)), t)
        assert abs(got - want) <= bnd, (t, got, want)
    assert np.array_equal(mx.diag(Xc), RM.diag(p, j, x, "d", M, N), equal_nan=True)


def test_margins_of_a_coo_with_repeated_triplets(gpu):
    """Matrix's reductions see the merged matrix: integer data, so every order of merging and summing is exact"""
    rng = np.random.default_rng(23)
    nnz = 3000
    i, j = rng.integers(0, 50, nnz).astype(np.int32), rng.integers(0, 30, nnz).astype(np.int32)
    x = rng.integers(-9, 10, nnz).astype(np.float64)
    D = np.zeros((50, 30))
    np.add.at(D, (i, j), x)
    assert nnz > np.count_nonzero(D)                     # repeated cells
    T = mx.dgTMatrix(i, j, x, (50, 30))
    assert np.array_equal(mx.rowSums(T), D.sum(axis=1)) and np.array_equal(mx.colSums(T), D.sum(axis=0))
    assert np.array_equal(mx.rowMeans(T), D.sum(axis=1) / 30.0) and np.array_equal(mx.colMeans(T), D.sum(axis=0) / 50.0)
    assert np.array_equal(mx.diag(T), np.diag(D)) and mx.norm(T, "M") == np.abs(D).max()
    assert mx.norm(T, "O") == np.abs(D).sum(axis=0).max() and mx.norm(T, "I") == np.abs(D).sum(axis=1).max()
    assert mx.norm(T, "F") == np.sqrt(np.square(D).sum())


@pytest.mark.parametrize("kind", ["d", "l", "n"])
def test_norm_and_diag(gpu, kind):
    X, (p, j, x) = operand(kind, seed=24)
    want_diag = RM.diag(p, j, x, kind, M, N)
    got_diag = mx.diag(X)
    assert got_diag.dtype == want_diag.dtype and np.array_equal(got_diag, want_diag, equal_nan=(kind == "d"))
    for t in RM.NORM_KINDS:                              # the NAs make every norm NaN
        if kind != "n":
            assert np.isnan(mx.norm(X, t)), t
    if kind == "d":
        x = np.where(np.isnan(x), -3.0, x)
    elif kind == "l":
        x = np.where(x == RM.NA_LOGICAL, 1, x).astype(np.int32)
    X = type(X)(p, j, x, (M, N))
    for t in RM.NORM_KINDS:
        want, bnd = RM.norm(p, j, x, kind, M, N, t)
        got = mx.norm(X, t)
        assert abs(got - want) <= (bnd if kind == "d" else 0.0), (t, got, want, bnd)
        assert mx.norm(X, [t, "zz"]) == got              # the first element counts
    assert mx.norm(X) == mx.norm(X, "O")
    with pytest.raises(mx.MatrixExtraError, match="single character"):
        mx.norm(X, 1)
    with pytest.raises(mx.MatrixExtraError, match="Invalid norm type. Allowed values:"):
        mx.norm(X, "E")
    with pytest.raises(mx.MatrixExtraError, match="spectral"):
        mx.norm(X, "2")


def test_norm_exact_data_and_empty_operands(gpu):
    p, j, _ = rand_csr(120, 90, 0.3, 25)
    x = np.random.default_rng(25).integers(-9, 10, size=j.size).astype(np.float64)
    X, D = mx.dgRMatrix(p, j, x, (120, 90)), csr_to_dense(p, j, x, 90)
    assert mx.norm(X, "F") == np.sqrt(np.square(D).sum())                 # the exact sum, one correctly rounded sqrt
    assert mx.norm(X, "1") == np.abs(D).sum(axis=0).max() and mx.norm(X, "i") == np.abs(D).sum(axis=1).max()
    assert mx.norm(X, "m") == 9.0
    z = np.zeros(1, dtype=np.int32)
    for Dim, pp in (((0, 5), z), ((5, 0), np.zeros(6, dtype=np.int32)), ((4, 4), np.zeros(5, dtype=np.int32))):
        E = mx.dgRMatrix(pp, np.zeros(0, dtype=np.int32), np.zeros(0), Dim)
        assert all(mx.norm(E, t) == 0.0 for t in RM.NORM_KINDS)
        assert np.array_equal(mx.diag(E), np.zeros(min(Dim))) and np.array_equal(mx.colSums(E), np.zeros(Dim[1]))
        assert np.array_equal(mx.rowSums(E), np.zeros(Dim[0]))


def test_export_level_calls_from_host_arrays(gpu):
    _, (p, j, x) = operand("d", seed=26)
    for op in RM.OPS:
        for axis in (0, 1):
            for na_rm in (False, True):
                got = exports.csr_margin_reduce(p, j, x, N, axis, op, na_rm)
                want, _, bnd = RM.margin(op, p, j, x, "d", M, N, axis == 0, na_rm)
                RM.assert_reduced(got, None, want, None, bnd, f"op {op} axis {axis} na_rm {na_rm}")
    _, (p, j, xl) = operand("l", seed=26)
    got = exports.csr_margin_reduce(p, j, xl, N, 1, RM.SUM, True, True, value_dtype=_lib.MX_LGL)
    assert np.array_equal(got, RM.margin(RM.SUM, p, j, xl, "l", M, N, False, True, True)[0])
    assert np.array_equal(exports.csr_margin_reduce(p, j, None, N, 0), np.diff(p).astype(np.float64))
    assert np.array_equal(exports.csr_diag(p, j, xl, N), RM.diag(p, j, xl, "l", M, N))
    assert np.array_equal(exports.csr_diag(p, j, None, N), RM.diag(p, j, None, "n", M, N))
    assert exports.csr_norm(p, j, None, N, "M") == 1.0 and exports.csr_norm(p, j, None, N, "F") == np.sqrt(j.size)
    assert exports.csr_norm(p, j, None, N, "I") == np.diff(p).max()
    with pytest.raises(_lib.MxError, match="type must be one of"):
        exports.csr_norm(p, j, None, N, "o")
    bad = j.copy()
    bad[5] = N
    with pytest.raises(_lib.MxError, match="column index outside"):
        exports.csr_margin_reduce(p, bad, x, N, 1)


def test_the_vignettes_gradient_step(gpu):
    """colMeans(X * v) on a 300 x 40 cbind(1, X) (vignettes/Introducing_MatrixExtra.Rmd:454-470), through the mirror
    and through device.col_reduce with the order of X serving the product, built once"""
    import torch
    from matrixextra_amd import device as dv
    p0, j0, x0 = rand_csr(M, N - 1, 0.15, 27)
    rows = np.repeat(np.arange(M), np.diff(p0))
    p = (p0 + np.arange(M + 1)).astype(np.int32)                          # one more entry per row: the intercept
    j, x = np.empty(j0.size + M, dtype=np.int32), np.empty(j0.size + M)
    at = p[:-1]
    body = np.ones(j.size, dtype=bool)
    body[at] = False
    j[at], x[at], j[body], x[body] = 0, 1.0, j0 + 1, x0
    X = mx.dgRMatrix(p, j, x, (M, N), [None, COLN])
    v = np.random.default_rng(28).normal(size=M)
    Y = X * v
    rows = np.repeat(np.arange(M), np.diff(p))
    assert np.array_equal(Y.p, p) and np.array_equal(Y.j, j) and np.array_equal(Y.x, x * v[rows])
    got = mx.colMeans(Y)
    assert got.names == COLN
    want, _, bnd = RM.margin(RM.SUM, p, j, Y.x, "d", M, N, False, mean=True)
    RM.assert_reduced(np.asarray(got), None, want, None, bnd, "colMeans(X * v) against fsum")
    # dense numpy: its own sum over the M cells of a column is one more summation order of the same products (zeros
    # add exactly), so it lies within the same gamma_M * sum|y| / M of the exact mean, plus the division's rounding
    D = csr_to_dense(p, j, x, N) * v[:, None]
    dense = D.mean(axis=0)
    slack = RM.gamma(M) * np.abs(D).sum(axis=0) / M + 2.0 * RM.U * np.abs(dense)
    assert np.all(np.abs(np.asarray(got) - dense) <= bnd + slack)
    assert abs(got[0] - v.mean()) <= bnd[0] + slack[0]                     # the intercept column: mean(v)

    dX = dv.DeviceCSR.from_host(p, j, x, N)
    order = dX.column_order()
    sums = []
    for step in range(3):                                                  # three gradients of one fit
        vs = v * (step + 1.0)
        dY = dv.DeviceCSR(dX.indptr, dX.indices, torch.from_numpy(x * vs[rows]).cuda(), M, N, dX.nnz)
        sums.append(dv.col_reduce(dY, "sum", order=dX.column_order()).cpu().numpy())
        assert dY._order is None and dY._order_builds == 0
    assert dX._order_builds == 1 and dX.column_order() is order            # the order was built only once
    assert np.array_equal(order[0].cpu().numpy(), np.argsort(j, kind="stable"))
    assert np.array_equal((sums[0] / M).view(np.uint64), np.asarray(got).view(np.uint64))   # the same kernel, the same bits
    for step in (1, 2):
        w, _, b = RM.margin(RM.SUM, p, j, x * (v * (step + 1.0))[rows], "d", M, N, False)
        RM.assert_reduced(sums[step], None, w, None, b, f"gradient {step}")
    own = dv.col_reduce(dv.DeviceCSR.from_host(p, j, Y.x, N), "sum").cpu().numpy()
    assert np.array_equal(own.view(np.uint64), sums[0].view(np.uint64))
    r, skipped = dv.row_reduce(dX, "abs_max", na_rm=True)
    assert np.array_equal(r.cpu().numpy(), RM.margin(RM.ABS_MAX, p, j, x, "d", M, N, True)[0]) and not skipped.any()
    assert dv.norm(dX, "O") == mx.norm(X, "O") and dv.norm(dX, "F") == mx.norm(X, "F")
    assert np.array_equal(dv.diag(dX).cpu().numpy(), RM.diag(p, j, x, "d", M, N))
