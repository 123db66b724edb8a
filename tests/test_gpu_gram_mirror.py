"""The one-triangle Gram product from the export (exports.csr_gram), the resident wrapper (device.gram) and the mirror:
crossprod(x) / tcrossprod(x) of matmul.py under options["mxgpu.spgemm_route"] together with
options["mxgpu.gram_symmetric"].  The export is compared with tests/gram_model.py bit for bit; the mirror's symmetric
result, expanded on the device, with the general route's result in p, indices and value bits.  Values are general
floats without NaN: the equality of the two triangles rests on the order of the sums, not on exact data."""
import itertools

import numpy as np
import pytest

import gram_model as GM
import matrixextra_amd as mx
from conftest import rand_csr
from matrixextra_amd import exports as G
from matrixextra_amd.matrices import options
from matrixextra_amd.structured import check_valid_structured, dsCMatrix, dsRMatrix

pytestmark = pytest.mark.gpu
M_, K_ = 40, 25
NA = mx.NA_INTEGER
UPLO = {"U": GM.UPPER, "L": GM.LOWER}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def values(kind, size, seed):
    rng = np.random.default_rng(seed)
    if kind == "d":
        return rng.normal(size=size) * 10.0 ** rng.integers(-3, 4, size=size)
    if kind == "l":
        return rng.choice(np.array([1, 1, 0, NA], dtype=np.int32), size=size)
    return None


def arrays(shape, seed, kind="d", sorted_cols=True):
    """(p, j, x) of a shape[0] x shape[1] CSR at density 0.3 with three empty rows and an empty column"""
    m, n = shape
    p, j, _ = rand_csr(m, n, 0.3, seed, sorted_cols=sorted_cols, empty_rows=(0, m // 2, m - 1))
    rows = np.repeat(np.arange(m), np.diff(p))
    keep = j != 3                                                       # column 3 stays empty
    p = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32)
    j = np.ascontiguousarray(j[keep])
    return p, j, values(kind, j.size, seed)


@pytest.fixture
def route():
    options["mxgpu.spgemm_route"] = True
    yield
    options.pop("mxgpu.spgemm_route", None)
    options.pop("mxgpu.gram_symmetric", None)


def symmetric(call, x):
    options["mxgpu.gram_symmetric"] = True
    try:
        return call(x)
    finally:
        options.pop("mxgpu.gram_symmetric", None)


# ---- the export ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", "dln")
@pytest.mark.parametrize("trans,uplo", list(itertools.product((0, 1), "UL")))
@pytest.mark.parametrize("shape", [(M_, K_), (K_, M_)])
def test_the_export_against_the_model(gpu, shape, trans, uplo, kind):
    p, j, x = arrays(shape, 31, kind)
    assert (np.diff(p) == 0).sum() >= 3 and 3 not in j
    res = G.csr_gram(p, j, x, shape, trans, uplo)
    wp, wj, wx = GM.gram(p, j, x, shape, trans, UPLO[uplo])
    n = shape[1] if trans else shape[0]
    assert res["indptr"].size == n + 1 and np.array_equal(res["indptr"], wp) and np.array_equal(res["indices"], wj)
    nan = np.isnan(wx)
    assert np.array_equal(np.isnan(res["values"]), nan) and np.array_equal(bits(res["values"][~nan]), bits(wx[~nan]))
    assert res["values"].dtype == np.float64 and (kind != "l" or nan.any())


def test_the_export_takes_unsorted_rows_for_the_transposed_side_on_the_left(gpu):
    """trans = 1 on unsorted rows: b_sorted comes from mxd_csr_rows_sorted on the upload, and nothing is trimmed"""
    p, j, x = arrays((M_, K_), 32, sorted_cols=False)
    assert not G.check_indices_are_sorted(p, j)
    for uplo in "UL":
        res = G.csr_gram(p, j, x, (M_, K_), 1, uplo)
        wp, wj, wx = GM.gram(p, j, x, (M_, K_), 1, UPLO[uplo])
        assert np.array_equal(res["indptr"], wp) and np.array_equal(res["indices"], wj)
        assert np.array_equal(bits(res["values"]), bits(wx))


def test_empty_results(gpu):
    z = lambda n: np.zeros(n + 1, np.int32)                             # noqa: E731
    e = np.zeros(0, np.int32)
    for dims, trans, n in (((0, 4), 0, 0), ((0, 4), 1, 4), ((6, 0), 1, 0), ((6, 4), 0, 6), ((6, 4), 1, 4)):
        res = G.csr_gram(z(dims[0]), e, None if dims[0] % 2 else np.zeros(0), dims, trans, "U")
        assert np.array_equal(res["indptr"], z(n)) and res["indices"].size == 0 and res["values"].size == 0


# ---- the mirror ----------------------------------------------------------------------------------------------------------
def names(tag, shape):
    return [["%sr%d" % (tag, r) for r in range(shape[0])], ["%sc%d" % (tag, c) for c in range(shape[1])]]


def operands():
    """name -> (operand, its sorted twin for the general route)"""
    shape = (M_, K_)
    p, j, x = arrays(shape, 33)
    ops = {"dgRMatrix": mx.dgRMatrix(p, j, x, shape, names("x", shape))}
    cp, ci, cx = arrays((K_, M_), 34)                                   # the CSC arrays of an M_ x K_ matrix
    ops["dgCMatrix"] = mx.dgCMatrix(cp, ci, cx, shape, names("c", shape))
    xl = values("l", j.size, 35)
    xl[xl == NA] = 1                                                    # NaN-free: stored TRUE and FALSE alone
    ops["lgRMatrix"] = mx.lgRMatrix(p, j, xl, shape, names("l", shape))
    ops["ngRMatrix"] = mx.ngRMatrix(p, j, None, shape, names("n", shape))
    rng = np.random.default_rng(36)
    T = np.triu(np.where(rng.random((K_, K_)) < 0.3, rng.normal(size=(K_, K_)), 0.0))
    r, c = np.nonzero(T)
    tp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=K_))]).astype(np.int32)
    ops["dsRMatrix"] = mx.dsRMatrix(tp, c, T[r, c], (K_, K_), [None, ["s%d" % k for k in range(K_)]], uplo="U")
    up, uj, ux = arrays(shape, 37, sorted_cols=False)
    ops["unsorted"] = mx.dgRMatrix(up, uj, ux, shape, names("u", shape))
    twins = dict(ops)
    twins["unsorted"] = mx.dgRMatrix(*GM.sort_rows(up, uj, ux), shape, names("u", shape))
    return {k: (ops[k], twins[k]) for k in ops}


CALL = {"crossprod": mx.crossprod, "tcrossprod": mx.tcrossprod}


def idx_of(o):
    """the minor indices of a compressed matrix of either layout"""
    return o.i if hasattr(o, "i") else o.j


@pytest.mark.parametrize("signature", sorted(CALL))
@pytest.mark.parametrize("name", ["dgRMatrix", "dgCMatrix", "lgRMatrix", "ngRMatrix", "dsRMatrix", "unsorted"])
def test_the_mirror_returns_the_symmetric_class_and_equals_the_general_route(gpu, route, name, signature):
    x, twin = operands()[name]
    if name == "unsorted":
        assert not G.check_indices_are_sorted(x.p, x.j) and G.check_indices_are_sorted(twin.p, twin.j)
    before = idx_of(x).copy()
    general = CALL[signature](twin)                                     # mxgpu.spgemm_route alone: today's general matrix
    out = symmetric(CALL[signature], x)
    assert np.array_equal(idx_of(x), before)                            # an unsorted operand is sorted in a copy
    cls = dsCMatrix if name == "dgCMatrix" else dsRMatrix
    n = x.Dim[1] if signature == "crossprod" else x.Dim[0]
    assert type(out) is cls and out.uplo == "U" and out.Dim == (n, n) == general.Dim
    assert type(general) is (mx.dgCMatrix if name == "dgCMatrix" else mx.dgRMatrix)
    assert out.Dimnames == general.Dimnames and out.x.dtype == np.float64
    if name != "dsRMatrix":
        dn = x.Dimnames[1] if signature == "crossprod" else x.Dimnames[0]
        assert out.Dimnames == [dn, dn]
    check_valid_structured(out)
    # as many stored entries as the upper triangle of the general result has
    gi = idx_of(general)
    major = np.repeat(np.arange(n), np.diff(general.p))
    upper = (gi <= major) if name == "dgCMatrix" else (gi >= major)     # a CSC's major index is the column
    assert out.idx.size == int(upper.sum()) == out.p[-1] == out.x.size
    assert not np.isnan(general.x).any()
    # expanded on the device, it is the general matrix: p, indices and value bits
    back = mx.as_csc_matrix(out) if name == "dgCMatrix" else mx.as_csr_matrix(out)
    assert type(back) is type(general) and np.array_equal(back.p, general.p) and np.array_equal(idx_of(back), gi)
    assert np.array_equal(bits(back.x), bits(general.x))


def test_with_the_option_off_the_result_is_the_general_matrix(gpu, route):
    x, _ = operands()["dgRMatrix"]
    assert not options.get("mxgpu.gram_symmetric", False)
    out = mx.crossprod(x)
    assert type(out) is mx.dgRMatrix and out.Dim == (K_, K_)
    rows = np.repeat(np.arange(K_), np.diff(out.p))
    assert (out.j < rows).any() and (out.j > rows).any()                # both triangles are stored
    options["mxgpu.gram_symmetric"] = False
    assert type(mx.tcrossprod(x)) is mx.dgRMatrix


def test_a_consumer_takes_the_symmetric_result(gpu, route):
    x, _ = operands()["dgRMatrix"]
    for call in CALL.values():
        general, out = call(x), symmetric(call, x)
        assert np.array_equal(bits(mx.rowSums(out)), bits(mx.rowSums(general)))
        assert np.array_equal(bits(mx.colSums(out)), bits(mx.colSums(general)))


# ---- the resident form ---------------------------------------------------------------------------------------------------
def test_the_resident_form_equals_the_export_on_one_column_order(gpu):
    from matrixextra_amd import device as dv
    p, j, x = arrays((M_, K_), 38)
    A = dv.DeviceCSR.from_host(p, j, x, K_)
    for trans, uplo in itertools.product((True, False), "UL"):
        for _ in range(2):
            Cd = dv.gram(A, trans=trans, uplo=uplo)
        n = K_ if trans else M_
        assert A._order_builds == 1 and Cd._sorted is True and (Cd.m, Cd.K) == (n, n)
        res = G.csr_gram(p, j, x, (M_, K_), trans, uplo)
        cp, cj, cx = Cd.to_host()
        assert np.array_equal(cp, res["indptr"]) and np.array_equal(cj, res["indices"]) and cx.size == Cd.nnz
        assert np.array_equal(bits(cx), bits(res["values"]))
    # the general product, with the same order: its triangle is the masked result
    full = dv.spgemm(A.transposed(), A)
    fp, fj, fx = full.to_host()
    tp, tj, tx = GM.triangle_of(fp, fj, fx, GM.UPPER)
    up = dv.spgemm(A.transposed(), A, uplo="U")
    gp, gj, gx = up.to_host()
    assert A._order_builds == 1 and np.array_equal(gp, tp) and np.array_equal(gj, tj) and np.array_equal(bits(gx), bits(tx))
    with pytest.raises(ValueError, match="uplo must be 'U' or 'L'"):
        dv.gram(A, uplo="x")
