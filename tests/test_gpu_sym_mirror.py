"""The symmetric and triangular classes on the GPU (matrixextra_amd/structured.py and what it is wired into): all
eight classes x uplo (x diag for the triangular ones) against a dense model built in numpy from the triplets.
Conversions, slices, sums and binds only copy or add integer-valued data and are compared exactly; the products use
the tolerances tests/test_gpu_parity.py uses for SpMM.  The operands are the reference's own `sy` and `tri`
(tests/testthat/test-slice.R:161-172, test-matmul.R:33-50 and :75-95) and a random 40 x 40 triangle.  Every test ends
by checking that its operands were not changed."""
import json

import numpy as np
import pytest

import matrixextra_amd as mx
import sym_model as SM

pytestmark = pytest.mark.gpu

F64_RTOL, F32_RTOL = 1e-12, 1e-5                     # as in tests/test_gpu_parity.py
CLASSES = {"dsRMatrix": mx.dsRMatrix, "lsRMatrix": mx.lsRMatrix, "nsRMatrix": mx.nsRMatrix, "dtRMatrix": mx.dtRMatrix,
           "ltRMatrix": mx.ltRMatrix, "ntRMatrix": mx.ntRMatrix, "dsCMatrix": mx.dsCMatrix, "dtCMatrix": mx.dtCMatrix}
FLIP = {"U": "L", "L": "U"}


def variants():
    out = []
    for name, cls in CLASSES.items():
        for uplo in SM.UPLOS:
            for diag in (("N",) if cls.symmetric else ("N", "U")):
                out.append((name, uplo, diag))
    return out


VARIANTS = variants()
vid = lambda v: "-".join(v)                           # noqa: E731


def triplets(source, strict):
    """(n, r, c) in the upper triangle, and the column names"""
    if source == "random":
        r, c = SM.random_upper(40, 3, 8, diagonal=True)
        lead = np.triu_indices(5)                     # a full leading block: no slice below selects nothing at all
        rc = np.unique(np.stack([np.concatenate([r, lead[0]]), np.concatenate([c, lead[1]])]), axis=1)
        r, c = rc[0], rc[1]
        n, names = 40, ["c%d" % k for k in range(40)]
    else:
        with open(SM.GOLDEN) as f:
            g = json.load(f)[source]
        n, r, c, names = g["n"], SM.rows_of(np.asarray(g["p"])), np.asarray(g["j"], dtype=np.int64), g.get("colnames")
    if strict:
        r, c = r[r != c], c[r != c]
    return n, r, c, names


def build(variant, source, with_na=False):
    """(X, dense, kind): the object and the dense float64 matrix it stands for (NA as nan)"""
    name, uplo, diag = variant
    cls = CLASSES[name]
    n, r, c, names = triplets(source, strict=diag == "U")
    if uplo == "L":
        r, c = c, r
    rng = np.random.default_rng(len(name) + n)
    kind = name[0]
    if kind == "d":
        v = rng.integers(1, 9, r.size).astype(np.float64)
    elif kind == "l":
        v = rng.choice(np.array([0, 1, SM.NA_LOGICAL], dtype=np.int32), r.size, p=[0.2, 0.6, 0.2]) if with_na \
            else rng.integers(0, 2, r.size).astype(np.int32)
    else:
        v = None
    dense = np.zeros((n, n))
    dv = 1.0 if v is None else np.where(v == SM.NA_LOGICAL, np.nan, v.astype(np.float64)) if kind == "l" else v
    dense[r, c] = dv
    if cls.symmetric:
        dense[c, r] = dv
    if diag == "U":
        dense[np.arange(n), np.arange(n)] = 1.0
    a, b = (r, c) if cls.layout == "R" else (c, r)                      # a CSC's slots are the CSR of the transpose
    order = np.lexsort((b, a))
    p = np.zeros(n + 1, dtype=np.int32)
    p[1:] = np.cumsum(np.bincount(a, minlength=n))
    X = cls(p, SM.i32(b[order]), None if v is None else v[order], (n, n), [None, names], uplo=uplo, diag=diag)
    return X, dense, kind


class Unchanged:
    """the operands' arrays and slots before and after"""

    def __init__(self, *objs):
        self.objs = objs
        self.before = [self.snap(o) for o in objs]

    @staticmethod
    def snap(o):
        arrays = {k: (getattr(o, k), None if getattr(o, k) is None else getattr(o, k).copy()) for k in ("p", "i", "j", "x")
                  if hasattr(o, k)}
        return arrays, o.Dim, [None if d is None else list(d) for d in o.Dimnames], getattr(o, "uplo", None), getattr(o, "diag", None)

    def check(self):
        for o, (arrays, Dim, Dimnames, uplo, diag) in zip(self.objs, self.before):
            for k, (obj, copy) in arrays.items():
                assert getattr(o, k) is obj, f"slot {k} was replaced"
                assert copy is None or np.array_equal(SM.bits(obj), SM.bits(copy)), f"slot {k} was written"
            assert (o.Dim, o.Dimnames, getattr(o, "uplo", None), getattr(o, "diag", None)) == (Dim, Dimnames, uplo, diag)


def csc_dense(C):
    return mx.t_shallow(C).toarray().T


def general_g(n, seed=3):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < 0.15
    D = np.where(mask, rng.integers(1, 9, (n, n)).astype(np.float64), 0.0)
    r, c = np.nonzero(mask)
    p = np.zeros(n + 1, dtype=np.int32)
    p[1:] = np.cumsum(mask.sum(axis=1))
    return mx.dgRMatrix(p, SM.i32(c), D[r, c], (n, n)), D


@pytest.mark.parametrize("source", ["reference", "random"])
@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_conversions(gpu, variant, source):
    source = ("sy" if CLASSES[variant[0]].symmetric else "tri") if source == "reference" else source
    X, dense, kind = build(variant, source, with_na=True)
    keep = Unchanged(X)
    R = mx.as_csr_matrix(X)
    assert type(R) is mx.dgRMatrix and R.Dim == X.Dim
    np.testing.assert_array_equal(R.toarray(), dense)
    if CLASSES[variant[0]].symmetric:
        assert R.Dimnames == [X.Dimnames[1], X.Dimnames[1]]
    else:
        assert R.Dimnames == X.Dimnames
    assert np.all(np.diff(R.j)[np.diff(SM.rows_of(R.p)) == 0] > 0)       # sorted input rows give sorted output rows
    Lg = mx.as_csr_matrix(X, logical=True)
    assert type(Lg) is mx.lgRMatrix
    np.testing.assert_array_equal(Lg.toarray(), np.where(np.isnan(dense), np.nan, (dense != 0).astype(np.float64)))
    Bn = mx.as_csr_matrix(X, binary=True)
    assert type(Bn) is mx.ngRMatrix and np.array_equal(Bn.p, R.p) and np.array_equal(Bn.j, R.j)
    Cc = mx.as_csc_matrix(X)
    assert type(Cc) is mx.dgCMatrix and Cc.Dim == X.Dim
    np.testing.assert_array_equal(csc_dense(Cc), dense)
    T = mx.as_coo_matrix(X)
    assert type(T) is mx.dgTMatrix
    np.testing.assert_array_equal(T.toarray(), dense)
    own = mx.as_coo_matrix(X, logical=kind == "l", binary=kind == "n")
    assert type(own) is {"d": mx.dgTMatrix, "l": mx.lgTMatrix, "n": mx.ngTMatrix}[kind] and own.i.size == R.j.size
    np.testing.assert_array_equal(X.toarray(), dense)
    keep.check()


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_transposes(gpu, variant):
    X, dense, _ = build(variant, "random")
    keep = Unchanged(X)
    D = mx.t_deep(X)
    assert type(D) is type(X) and D.uplo == FLIP[X.uplo] and getattr(D, "diag", None) == getattr(X, "diag", None)
    np.testing.assert_array_equal(D.toarray(), dense.T)
    assert D.Dimnames == [X.Dimnames[1], X.Dimnames[0]]
    if variant[0] in ("dsRMatrix", "dtRMatrix", "dsCMatrix", "dtCMatrix"):
        S = mx.t_shallow(X)
        assert S.idx is X.idx and S.uplo == FLIP[X.uplo]
        np.testing.assert_array_equal(S.toarray(), dense.T)
    keep.check()


@pytest.mark.parametrize("source", ["reference", "random"])
@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_products(gpu, variant, source):
    """test-matmul.R:33-50 (matrix %*% dsC / dtC) and :53-96 (tcrossprod(matrix, dsR / dtR)), float32 included"""
    cls = CLASSES[variant[0]]
    source = ("sy" if cls.symmetric else "tri") if source == "reference" else source
    X, dense, _ = build(variant, source)
    n = X.Dim[0]
    rng = np.random.default_rng(1)
    A = np.where(rng.random((20, n)) < 0.4, np.round(rng.normal(size=(20, n)), 2), 0.0)   # rsparsematrix(20, n, .4)
    keep = Unchanged(X)
    if cls.layout == "C":
        got, got32, want = A @ X, mx.float32(A) @ X, A @ dense
        assert got.Dimnames[1] == X.Dimnames[1]
    else:
        got, got32, want = mx.tcrossprod(A, X), mx.tcrossprod(mx.float32(A), X), A @ dense.T
        also = mx.tcrossprod(X, A)                                       # RsparseMatrix on the left
        np.testing.assert_allclose(np.asarray(also), dense @ A.T, rtol=F64_RTOL, atol=1e-13)
        np.testing.assert_allclose(np.asarray(X @ A.T), dense @ A.T, rtol=F64_RTOL, atol=1e-13)
    np.testing.assert_allclose(np.asarray(got), want, rtol=F64_RTOL, atol=1e-13)
    assert isinstance(got32, mx.float32)
    np.testing.assert_allclose(got32.Data.astype(np.float64), want, rtol=F32_RTOL, atol=1e-5)
    keep.check()


def as_float(v):
    if isinstance(v, (bool, np.bool_)):
        return float(v)
    return np.nan if (isinstance(v, (int, np.integer)) and v == SM.NA_LOGICAL) else float(v)


@pytest.mark.parametrize("source", ["reference", "random"])
@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_slices(gpu, variant, source):
    """the five slices and two scalar lookups of test-slice.R:212-239 (0-based here)"""
    cls = CLASSES[variant[0]]
    source = ("sy" if cls.symmetric else "tri") if source == "reference" else source
    X, dense, kind = build(variant, source)
    keep = Unchanged(X)
    for key in [(slice(0, 3), slice(None)), ([1, 0, 2], slice(None)), (slice(0, 3), slice(1, 4)),
                (slice(0, 3), [2, 1, 3]), ([1, 0, 2], [2, 1, 3])]:
        got = X[key]
        assert isinstance(got, mx.RsparseMatrix), key
        if cls.layout == "R":
            assert type(got) is {"d": mx.dgRMatrix, "l": mx.lgRMatrix, "n": mx.ngRMatrix}[kind]
        rows, cols = key
        want = dense[rows, :][:, cols]
        assert got.Dim == want.shape
        np.testing.assert_array_equal(got.toarray(), want, err_msg=str(key))
    if cls.layout == "R":
        n = X.Dim[0]
        mx.options["mxgpu.slice_drop_route"] = True
        try:
            cells = [(3, 3)] + ([(6, 5), (5, 6)] if n >= 6 else []) + [(1, 2), (2, 1), (1, 1), (n, n)]
            for i, j in cells:
                got = mx.subset_csr(X, i, j, drop=True)
                assert as_float(got) == dense[i - 1, j - 1], (i, j)
                one = mx.subset_csr(X, i, j, drop=False)
                assert isinstance(one, mx.RsparseMatrix) and one.Dim == (1, 1) and one.toarray()[0, 0] == dense[i - 1, j - 1]
        finally:
            mx.options.pop("mxgpu.slice_drop_route", None)
        T = mx.subset_coo(X, np.array([2, 1, 3], dtype=np.int32), np.array([3, 2, 4], dtype=np.int32), drop=False)
        assert isinstance(T, mx.TsparseMatrix)
        np.testing.assert_array_equal(T.toarray(), dense[[1, 0, 2], :][:, [2, 1, 3]])
    keep.check()


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_arithmetic_with_a_dgRMatrix(gpu, variant):
    X, dense, _ = build(variant, "random")
    G, Gd = general_g(X.Dim[0])
    keep = Unchanged(X, G)
    for got, want in [(X + G, dense + Gd), (G + X, Gd + dense), (X - G, dense - Gd), (G - X, Gd - dense),
                      (X * G, dense * Gd), (G * X, Gd * dense)]:
        assert isinstance(got, mx.RsparseMatrix)
        np.testing.assert_array_equal(got.toarray(), want)
    if variant[0] in ("dsRMatrix", "dtRMatrix"):                          # the vector operators of a numeric CSR
        v = np.arange(1.0, X.Dim[0] + 1.0)
        np.testing.assert_array_equal((X * v).toarray(), dense * v[:, None])      # a vector recycles down the columns
        np.testing.assert_array_equal((v * X).toarray(), dense * v[:, None])
        np.testing.assert_array_equal((X / 2.0).toarray(), dense / 2.0)
    keep.check()


@pytest.mark.parametrize("variant", [v for v in VARIANTS if CLASSES[v[0]].layout == "R"], ids=vid)
def test_rbind_csr(gpu, variant):
    X, dense, kind = build(variant, "random")
    G, Gd = general_g(X.Dim[0])
    keep = Unchanged(X, G)
    two = mx.rbind_csr(X, G)
    assert type(two) is mx.dgRMatrix and two.Dim == (2 * X.Dim[0], X.Dim[1])
    np.testing.assert_array_equal(two.toarray(), np.vstack([dense, Gd]))
    three = mx.rbind_csr(G, X, X)
    np.testing.assert_array_equal(three.toarray(), np.vstack([Gd, dense, dense]))
    own = mx.rbind_csr(X, X, X)
    assert type(own) is {"d": mx.dgRMatrix, "l": mx.lgRMatrix, "n": mx.ngRMatrix}[kind]
    np.testing.assert_array_equal(own.toarray(), np.vstack([dense] * 3))
    np.testing.assert_array_equal(mx.rbind2(X, G).toarray(), np.vstack([dense, Gd]))
    np.testing.assert_array_equal(mx.cbind2(G, X).toarray(), np.hstack([Gd, dense]))
    if not CLASSES[variant[0]].symmetric and variant[2] == "N":          # passes through unexpanded: the same arrays
        same = mx.as_csr_matrix(X, logical=kind == "l", binary=kind == "n")
        assert same.p is X.p and same.j is X.j and same.x is X.x
    keep.check()


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_reductions(gpu, variant):
    X, dense, _ = build(variant, "random")
    keep = Unchanged(X)
    np.testing.assert_array_equal(np.asarray(mx.rowSums(X)), dense.sum(axis=1))
    np.testing.assert_array_equal(np.asarray(mx.colSums(X)), dense.sum(axis=0))
    assert mx.norm(X, "O") == np.abs(dense).sum(axis=0).max()
    np.testing.assert_array_equal(np.asarray(mx.diag(X), dtype=np.float64), np.diag(dense))
    keep.check()


def test_invalid_triangles_are_refused(gpu):
    """this build's own messages: an entry outside the stated triangle, and a stored diagonal under diag = "U" """
    X, _, _ = build(("dsRMatrix", "U", "N"), "random")
    X.uplo = "L"
    with pytest.raises(mx.MatrixExtraError, match="lie outside the triangle that 'uplo' names"):
        mx.as_csr_matrix(X)
    T, _, _ = build(("dtRMatrix", "U", "N"), "random")
    T.diag = "U"
    with pytest.raises(mx.MatrixExtraError, match="'diag' is \"U\""):
        mx.check_valid_matrix(T)
    C, _, _ = build(("dsCMatrix", "L", "N"), "random")
    mx.check_valid_matrix(C)
    C.uplo = "U"
    with pytest.raises(mx.MatrixExtraError, match="lie outside the triangle"):
        mx.as_csc_matrix(C)


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("uplo", SM.UPLOS)
def test_device_resident_operands(gpu, uplo, kind):
    """matrixextra_amd.device: the expansions and the check on a DeviceCSR, against the model bit for bit"""
    from matrixextra_amd import device as D
    n, p, j, x = SM.case("n300-crosses-the-tiles", uplo, kind)
    A = D.DeviceCSR.from_host(p, j, x, n)
    G = D.csr_symmetric_to_general(A, uplo)
    want = SM.symmetric_to_general(p, j, x, uplo)
    got = G.to_host()
    assert G.nnz == want[1].size and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (x is None and got[2] is None) or np.array_equal(SM.bits(got[2]), SM.bits(want[2]))
    on_diagonal = int(np.count_nonzero(j == SM.rows_of(p)))
    assert D.csr_triangle_check(A, uplo) == 0 and D.csr_triangle_check(A, uplo, strict=True) == on_diagonal
    keep = j != SM.rows_of(p)
    sp = np.zeros(n + 1, dtype=np.int32)
    sp[1:] = np.cumsum(np.bincount(SM.rows_of(p)[keep], minlength=n))
    sx = None if x is None else x[keep]
    U = D.csr_unit_triangular_to_general(D.DeviceCSR.from_host(sp, j[keep], sx, n), uplo)
    want = SM.unit_triangular_to_general(sp, j[keep], sx, kind, uplo)
    got = U.to_host()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (x is None and got[2] is None) or np.array_equal(SM.bits(got[2]), SM.bits(want[2]))
    assert np.array_equal(A.to_host()[1], j)
