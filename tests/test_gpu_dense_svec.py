"""`matrix * sparseVector` and the COO * dense gather on the device (csrc/densevec.hip): the exports
against what the reference's own compiled code returned (tests/golden/dense_svec_golden.npz) and against the numpy
model that the fixture and the live reference pin (tests/dense_svec_model.py), then device.dense_by_svec on tensors and
the Python mirror of R/operators.R:400-483 and :1641-1705.

Bars: bit for bit, NaN payloads included; every value is a copy, a constant or one IEEE multiplication.  Where both
factors of a product are NaN only NaN-ness is compared, on at most 5 % of a case (dense_svec_model.same).  The
deviations that DESIGN.md declares are handled by name (dense_svec_model.compare_svec): at the cells of deviation 2
the fixture must hold (double)NA_INTEGER and the device NA_real_; under deviation 5 (route C keeping NAs: the
reference loses the vector after its first recycle segment) the first segment is compared with the fixture and the
whole result with the model.  With an unsorted vector and NAs ignored, the CSR routes of the reference lay the rows
out in the vector's order under a row-ordered indptr; the device writes a CSR in row order, which is what the model
holds (deviation 6).

Shapes: the fill's tile is 64 x 64, so rows and columns run over {1, 63, 64, 65, 130} x {1, 2, 63, 64, 65}, with every
length of {cells, nrows, nrows/2, nrows/5, 7, nrows+3} whose route holds, and one case of many workgroups."""
import numpy as np
import pytest

import dense_svec_model as M
import refpin

import matrixextra_amd as mx
from matrixextra_amd import matrices

pytestmark = pytest.mark.gpu

RECORDS, _META = refpin.load(M.PATH)
NA_REAL_BITS = M.bits(np.array([M.NA_REAL]))[0]


def _deviates(rec):
    X, ii, length, keep = rec.args[0], rec.args[1], int(rec.args[3]), bool(rec.args[4])
    named = M.int_na_tail_cells(M.KIND_OF_FN[rec.fn], X, ii, length, keep)
    return (named is not None and bool(named.any())) or M.recycles_under_keep(*X.shape, ii.size, length, keep)


@pytest.mark.parametrize("rec", RECORDS, ids=[f"{n:03d}-{r!r}" for n, r in enumerate(RECORDS)])
def test_hip_reproduces_the_reference_run(gpu, rec):
    from matrixextra_amd import exports as G
    assert refpin.has(G, rec.fn), f"matrixextra_amd.exports has no {rec.fn}"
    got, live = refpin.replay(G, rec)
    assert not isinstance(got, Exception), f"{rec!r}: raised {got!r}"
    if rec.fn in M.COO_KIND_OF_FN:
        refpin.compare(rec, got, live, device=True)
        return M.compare_coo(rec.args, rec.fn, got, rec.out, repr(rec))
    if not _deviates(rec):
        refpin.compare(rec, got, live, device=True)
    for k, a in enumerate(rec.args):
        if isinstance(a, np.ndarray):
            refpin.exact(live[k], a, f"{rec!r} argument {k} after the call")
    M.compare_svec(rec.fn, rec.args, got, rec.out, repr(rec))


@pytest.mark.parametrize("keep", (False, True), ids=("ignore", "keep"))
@pytest.mark.parametrize("kind", M.KINDS)
def test_every_shape_length_and_pattern_against_the_model(gpu, kind, keep):
    from matrixextra_amd import exports as G
    n, routes = 0, set()
    for nrows in M.NROWS:
        for ncols in M.NCOLS:
            for length, rt in M.lengths_for(nrows, ncols):
                for pattern in M.PATTERNS:
                    X, ii, xx = M.svec_case(kind, nrows, ncols, length, pattern, 9000 + n)
                    n += 1
                    got = getattr(G, M.SVEC_FN[kind])(X, ii, xx, length, int(keep))
                    want, both = M.model(kind, X, ii, xx, length, keep)
                    M.compare_results(got, want, both, f"{kind} {nrows}x{ncols} L{length}{rt} {pattern} keep={keep}")
                    routes.add(rt)
    assert routes == set("ABCD") and n > 500


@pytest.mark.parametrize("keep", (False, True), ids=("ignore", "keep"))
@pytest.mark.parametrize("kind", M.KINDS)
def test_many_workgroups(gpu, kind, keep):
    """4099 x 257 with length = nrows: 65 row tiles x 5 column tiles, 17 blocks of counts, a scan over 4099 rows."""
    from matrixextra_amd import exports as G
    X, ii, xx = M.svec_case(kind, 4099, 257, 4099, "some", 777)
    got = getattr(G, M.SVEC_FN[kind])(X, ii, xx, 4099, int(keep))
    want, both = M.model(kind, X, ii, xx, 4099, keep)
    assert want["values"].size > 400000
    M.compare_results(got, want, both, f"{kind} 4099x257 keep={keep}")


def test_signs_of_zero_and_the_daxpy_rule(gpu):
    """0 and -1 against zero cells: route C without NAs is daxpy's 0.0 + value * X (+0.0, and +0.0 for a value of 0
    whatever X holds); route B and the other kinds multiply directly and keep -0.0."""
    from matrixextra_amd import exports as G
    X = np.asfortranarray(np.array([[0.0, 1.0], [0.0, np.nan], [0.0, 2.0], [0.0, np.inf], [0.0, -0.0], [0.0, 3.0]]))
    ii, xx = np.array([1, 2, 3], dtype=np.int32), np.array([-1.0, 0.0, -2.0])
    c = G.multiply_elemwise_dense_by_svec_numeric(X, ii, xx, 3, 0)["values"].reshape(6, 2)
    assert not np.signbit(c[[0, 2, 4, 5], 0]).any() and (M.bits(c[[1, 4]]) == 0).all()      # rows 1 and 4: value 0
    assert c[3, 1] == -np.inf and c[0, 1] == -1.0 and c[5, 1] == -6.0
    b = G.multiply_elemwise_dense_by_svec_numeric(X, ii, xx, 6, 0)["values"].reshape(3, 2)
    assert np.signbit(b[[0, 2], 0]).all() and np.isnan(b[1, 1]) and not np.signbit(b[1, 0])
    f = G.multiply_elemwise_dense_by_svec_float32(X.astype(np.float32), ii, xx, 3, 0)["values"].reshape(6, 2)
    assert np.signbit(f[[0, 2, 3, 5], 0]).all() and np.isnan(f[1, 1])                        # float32: no daxpy
    for args in ((X, ii, xx, 3, 0), (X, ii, xx, 6, 0)):
        M.compare_results(G.multiply_elemwise_dense_by_svec_numeric(*args), *M.model("numeric", *args), "signs")


def test_repeated_positions(gpu):
    """Not a valid sparseVector, but bounded and deterministic: the dense routes take the last entry of a position
    (the reference's overwriting scatter), the CSR routes the first (its lower_bound skip)."""
    from matrixextra_amd import exports as G
    X = np.asfortranarray(np.arange(1.0, 9.0).reshape(4, 2))
    ii, xx = np.array([2, 2, 3], dtype=np.int32), np.array([10.0, 100.0, 2.0])
    d = G.multiply_elemwise_dense_by_svec_numeric(X, ii, xx, 8, 1)["X_dense"]
    assert d[1, 0] == X[1, 0] * 100.0 and d[2, 0] == X[2, 0] * 2.0 and d[0, 0] == 0.0
    c = G.multiply_elemwise_dense_by_svec_numeric(X, ii, xx, 4, 1)
    assert c["indptr"].tolist() == [0, 0, 2, 4, 4] and c["values"].tolist() == [X[1, 0] * 10, X[1, 1] * 10, X[2, 0] * 2, X[2, 1] * 2]


# ----------------------------------------------------------------------------- COO * dense
@pytest.mark.parametrize("nnz", (0, 1, 65, 4099))
@pytest.mark.parametrize("kind", ("numeric", "integer", "logical", "float32", "and"))
def test_coo_by_dense_against_the_model(gpu, kind, nnz):
    from matrixextra_amd import exports as G
    X, ii, jj, xx = M.coo_case(kind, nnz, 3100 + nnz, nrows=130, ncols=65)
    got = getattr(G, M.COO_FN[kind])(X, ii, jj, xx)
    val, _ = M.coo_model(kind, X, ii, jj, xx)
    M.compare_coo([X, ii, jj, xx], M.COO_FN[kind], got, dict(row=ii, col=jj, val=val), f"{kind} nnz={nnz}")
    assert got["row"] is not ii and got["col"] is not jj
    if nnz > 1:
        na = X[ii, jj] == M.NA_INT if kind in ("integer", "logical") else np.zeros(nnz, dtype=bool)
        assert kind not in ("integer", "logical") or (na.any() and (M.bits(got["val"][na]) == NA_REAL_BITS).all())
        assert len(set(zip(ii.tolist(), jj.tolist()))) < nnz          # a repeated triplet


def test_coo_mirror_under_the_option(gpu, monkeypatch):
    monkeypatch.setitem(matrices.options, "mxgpu.coo_dense_route", True)
    X, ii, jj, xx = M.coo_case("integer", 65, 3300, nrows=9, ncols=7)
    X[X == M.NA_INT] = 5                                      # without NA: the gather
    T = mx.dgTMatrix(ii, jj, xx, (9, 7))
    for out in (T * X, X * T):
        assert isinstance(out, mx.dgTMatrix) and out.Dim == (9, 7)
        assert np.array_equal(out.i, ii) and np.array_equal(out.j, jj) and out.i is not T.i
        M.same(out.x, M.coo_model("integer", X, ii, jj, xx)[0], np.zeros(65, dtype=bool), "T * integer matrix")
    B = X != 0
    M.same((T * B).x, M.coo_model("logical", B.astype(np.int32), ii, jj, xx)[0], np.zeros(65, dtype=bool), "T * logical matrix")
    # with an NA while NAs are kept: the CSC route, which adds the NA cells outside the pattern
    Xna = X.copy()
    Xna[8, 6] = M.NA_INT
    out = T * Xna
    assert isinstance(out, mx.dgCMatrix) and out.Dim == (9, 7)
    # lgTMatrix & matrix: every `&` goes to the vector route (R/operators.R:402-403), as without the option
    L = mx.lgTMatrix(ii, jj, np.where(np.isnan(xx), M.NA_INT, 1).astype(np.int32), (9, 7))
    monkeypatch.setitem(matrices.options, "mxgpu.coo_dense_route", False)
    before = L & B
    monkeypatch.setitem(matrices.options, "mxgpu.coo_dense_route", True)
    after = L & B
    assert type(after) is type(before) is mx.lgTMatrix and np.array_equal(after.x, before.x)
    want = M.coo_model("and", B.astype(np.int32), ii, jj, L.x)[0]
    np.testing.assert_array_equal(after.x, want)


# ----------------------------------------------------------------------------- the mirror: v * M and M * v
@pytest.fixture
def opts(monkeypatch):
    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setitem(matrices.options, "MatrixExtra." + k, v)
    return set_


def test_mirror_matrix_times_svec(gpu, opts):
    X, ii, xx = M.svec_case("numeric", 65, 3, 65, "some", 4400)
    perm = np.random.default_rng(5).permutation(ii.size)
    names = [[f"r{r}" for r in range(65)], ["a", "b", "c"]]
    D = mx.DenseMatrix(X, names)
    want, both = M.model("numeric", X, ii, xx, 65, True)
    v = mx.dsparseVector(ii[perm], xx[perm], 65)                          # unsorted: sorted in a copy
    for out in (D * v, v * D, X * v):
        assert isinstance(out, mx.dgRMatrix) and out.Dim == (65, 3)
        M.compare_results(dict(indptr=out.p, indices=out.j, values=out.x), want, both, "M * v")
    assert (D * v).Dimnames == names and (X * v).Dimnames == [None, None]
    assert np.array_equal(v.i, ii[perm])
    opts(inplace_sort=True)
    out = D * v                                                           # sorted in place
    assert np.array_equal(v.i, ii) and M.bits(v.x).tolist() == M.bits(xx).tolist()
    M.compare_results(dict(indptr=out.p, indices=out.j, values=out.x), want, both, "M * v, in place")
    opts(inplace_sort=False, ignore_na=True)
    u = mx.dsparseVector(ii[perm], xx[perm], 65)                          # unsorted and left so: rows still in row order
    out = D * u
    want0, both0 = M.model("numeric", X, ii[perm], xx[perm], 65, False)
    assert np.array_equal(u.i, ii[perm]) and want0["values"].size < want["values"].size
    M.compare_results(dict(indptr=out.p, indices=out.j, values=out.x), want0, both0, "M * v, NAs ignored")
    opts(ignore_na=False)

    # dense results come back as they are, without dimnames
    for length in (195, 7):
        Xd, i2, x2 = M.svec_case("numeric", 65, 3, length, "some", 4500 + length)
        out = mx.DenseMatrix(Xd, names) * mx.dsparseVector(i2[::-1].copy(), x2[::-1].copy(), length)
        assert type(out) is np.ndarray and out.shape == (65, 3) and out.flags.f_contiguous
        w, b = M.model("numeric", Xd, i2, x2, length, True)
        M.same(out, w["X_dense"], b, f"dense route, length {length}")


def test_mirror_kinds_and_empty_operands(gpu):
    for kind in ("integer", "logical", "float32"):
        X, ii, xx = M.svec_case(kind, 64, 65, 32, "some", 4600)
        v = mx.dsparseVector(ii, xx, 32)
        left = mx.float32(X) if kind == "float32" else (X != 0) if kind == "logical" else X
        if kind == "logical":
            X = (X != 0).astype(np.int32)
        want, both = M.model(kind, X, ii, xx, 32, True)
        for out in (left * v, v * left):
            assert isinstance(out, mx.dgRMatrix) and out.Dim == (64, 65)
            M.compare_results(dict(indptr=out.p, indices=out.j, values=out.x), want, both, f"{kind} matrix * v")
    w = mx.isparseVector([2, 1], [3, mx.NA_INTEGER], 4)                    # another kind of vector: NA_integer_ -> NA_real_
    out = np.asfortranarray(np.arange(1.0, 9.0).reshape(4, 2)) * w
    assert out.p.tolist() == [0, 2, 4, 4, 4] and (M.bits(out.x[:2]) == NA_REAL_BITS | (1 << 51)).all() and out.x[2:].tolist() == [9.0, 12.0]
    for out in (np.ones((0, 3)) * mx.dsparseVector([1], [2.0], 4), mx.dsparseVector([], [], 0) * np.ones((2, 3))):
        assert out.shape == (1, 1) and np.isnan(out[0, 0])


# ----------------------------------------------------------------------------- device.dense_by_svec on tensors
@pytest.mark.parametrize("kind", M.KINDS)
def test_device_dense_by_svec(gpu, kind):
    import torch
    from matrixextra_amd import device
    dev = torch.device("cuda:0")
    for nrows, ncols, length in ((130, 65, 130), (130, 65, 26), (65, 64, 65 * 64), (65, 64, 7)):
        for keep in (False, True):
            X, ii, xx = M.svec_case(kind, nrows, ncols, length, "some", 4700 + length)
            Xt = torch.from_numpy(np.ascontiguousarray(X)).to(dev)         # row-major on the device: any strides do
            got = device.dense_by_svec(Xt, torch.from_numpy(ii).to(dev), torch.from_numpy(xx).to(dev), length,
                                       keep_na=keep, logical=kind == "logical")
            want, both = M.model(kind, X, ii, xx, length, keep)
            what = f"device {kind} {nrows}x{ncols} L{length} keep={keep}"
            if "X_dense" in want:
                assert tuple(got.shape) == (nrows, ncols) and got.dtype == torch.float64
                M.same(np.asfortranarray(got.cpu().numpy()), want["X_dense"], both, what)
            else:
                p, j, x = (t.cpu().numpy() for t in got)
                M.compare_results(dict(indptr=p, indices=j, values=x), want, both, what)
    Xt = torch.ones((4, 2), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="inside 1..4"):
        device.dense_by_svec(Xt, torch.tensor([5], dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float64, device=dev), 4)
    with pytest.raises(ValueError, match="float64"):
        device.dense_by_svec(Xt, torch.tensor([1], dtype=torch.int32, device=dev), torch.ones(1, device=dev), 4)
    b = device.dense_by_svec(Xt > 0, torch.tensor([1], dtype=torch.int32, device=dev), torch.full((1,), 3.0, dtype=torch.float64, device=dev), 4)
    assert b[0].tolist() == [0, 2, 2, 2, 2] and b[2].tolist() == [3.0, 3.0]
