"""rbind / cbind on the device, every route of matrixextra_amd/bind.py once per kind combination at the shapes of the
reference's own tests (10 x 3, 100 x 35: test-rbind.R:8, test-cbind.R).  The COO concat, the sparse vector as a column
of a CSR and the dense-vector compaction are checked exactly against numpy constructions written here; the routes
whose structure the reference leaves to Matrix are checked by dense equality, as test-rbind.R:24-50 does."""
import numpy as np
import pytest
import torch

import matrixextra_amd as mx
from bind_cases import NA, dev_cbind_svec, dev_coo_rbind, same_csr, same_values
from conftest import rand_csr
from matrixextra_amd import device as D
from matrixextra_amd import exports as G
from matrixextra_amd._lib import MX_F64, MX_I32, MX_LGL
from matrixextra_amd.matrices import (dgCMatrix, dgRMatrix, dgTMatrix, dsparseVector, isparseVector, lgRMatrix,
                                      lgTMatrix, lsparseVector, ngRMatrix, ngTMatrix, nsparseVector, t_shallow)

pytestmark = pytest.mark.gpu
SHAPES = [(10, 3), (100, 35)]
CSR = {"d": dgRMatrix, "l": lgRMatrix, "n": ngRMatrix}
COO = {"d": dgTMatrix, "l": lgTMatrix, "n": ngTMatrix}
SVEC = {"d": dsparseVector, "i": isparseVector, "l": lsparseVector, "n": nsparseVector}


# ----------------------------------------------------------------------------------------------- operands
def R(kind, m, n, seed, names=False):
    """names: False, "rows" or True (rows and columns)"""
    p, j, x = rand_csr(m, n, 0.4, seed, dtype=kind, empty_rows=(1,) if m > 1 else ())
    if kind == "d":
        x[::4] = np.nan
    dn = [[f"r{k}" for k in range(m)], [f"c{k}" for k in range(n)] if names is True else None] if names else None
    return CSR[kind](p, j, x, (m, n), dn)


def T(kind, m, n, seed, dup=False):
    """triplets in a shuffled order; dup: one of them repeated"""
    A = R(kind, m, n, seed)
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(m, dtype=np.int32), np.diff(A.p))
    order = rng.permutation(np.concatenate([np.arange(i.size), [0] if dup else []]).astype(np.int64))
    return COO[kind](i[order], A.j[order], None if A.x is None else A.x[order], (m, n))


def Cm(m, n, seed):
    A = R("d", n, m, seed)
    return dgCMatrix(A.p, A.j, A.x, (m, n))


def V(kind, length, seed, n=None, shuffle=False):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, length + 1)) if n is None else n
    i = np.sort(rng.permutation(length)[:n]).astype(np.int32) + 1
    if shuffle:
        i = rng.permutation(i).astype(np.int32)
    if kind == "n":
        x = None
    elif kind == "d":
        x = np.round(rng.normal(size=n), 2)
        x[::3] = np.nan
        x[1::3] = 0.0
    else:
        x = rng.integers(0, 2, n).astype(np.int32) if kind == "l" else rng.integers(-3, 4, n).astype(np.int32)
        x[::3] = NA
    return SVEC[kind](i, x, length)


def dense(x):
    """as.matrix: NA -> nan, a pattern entry -> 1, repeated triplets summed; a sparse vector is a 1-d array"""
    if isinstance(x, dgCMatrix):
        return t_shallow(x).toarray().T
    return x.toarray()


def pad(a, shape):
    out = np.zeros(shape)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def kind_of(*xs):
    ks = ["n" if isinstance(x, (ngRMatrix, ngTMatrix, nsparseVector)) else
          "l" if isinstance(x, (lgRMatrix, lgTMatrix, lsparseVector)) else "d" for x in xs]
    return "n" if all(k == "n" for k in ks) else "l" if all(k in "nl" for k in ks) else "d"


def convert(x, n, src, out, vec):
    """values of one operand in the output's kind: the table of src/rbind.cpp:72-166, written out"""
    if out == "n":
        return None
    if x is None:
        return np.ones(n, np.float64 if out == "d" else np.int32)
    if out == "d":
        if src == "d":
            return x
        v = (x != 0).astype(np.float64) if (src == "l" and vec) else x.astype(np.float64)
        return np.where(x == NA, np.nan, v)
    if src == "d":
        return np.where(np.isnan(x), NA, (x != 0).astype(np.int32)).astype(np.int32)
    if src == "i":
        return np.where(x == NA, NA, (x != 0).astype(np.int32)).astype(np.int32)
    return x


def letter(x):
    return {dsparseVector: "d", isparseVector: "i", lsparseVector: "l", nsparseVector: "n"}.get(
        type(x), kind_of(x))


# ----------------------------------------------------------------------------------------------- COO concat, exact
def coo_expected(ops, offsets, out):
    ii, jj, xx = [], [], []
    for o, off in zip(ops, offsets):
        vec = isinstance(o, mx.sparseVector)
        n = o.i.size
        ii.append(np.full(n, off, np.int32) if vec else o.i + np.int32(off))
        jj.append(o.i - 1 if vec else o.j)
        xx.append(convert(o.x, n, letter(o), out, vec))
    cat = np.concatenate
    return dict(ii=cat(ii), jj=cat(jj), xx=None if out == "n" else cat(xx))


def coo_check(got, want, cls, Dim):
    assert type(got) is cls and got.Dim == Dim
    np.testing.assert_array_equal(got.i, want["ii"])
    np.testing.assert_array_equal(got.j, want["jj"])
    same_values(got.x, want["xx"])


@pytest.mark.parametrize("m, n", SHAPES)
@pytest.mark.parametrize("kx", "dln")
@pytest.mark.parametrize("ky", "dln")
def test_rbind2_coo(gpu, m, n, kx, ky):
    x, y = T(kx, m, n, 1, dup=True), T(ky, m + 3, n + 2, 2, dup=True)
    out = kind_of(x, y)
    want = coo_expected([x, y], [0, m], out)
    coo_check(mx.rbind2(x, y), want, COO[out], (2 * m + 3, n + 2))
    ops = [(("dln".index(kx)), x.i, x.j, x.x, m), (("dln".index(ky)), y.i, y.j, y.x, m + 3)]
    got = dev_coo_rbind(ops, "dln".index(out))
    np.testing.assert_array_equal(got["ii"], want["ii"])
    np.testing.assert_array_equal(got["jj"], want["jj"])
    same_values(got["xx"], want["xx"])
    # cbind2 of T operands is the same concat between two t_shallow (R/cbind.R:20-22)
    z = mx.cbind2(t_shallow(x), t_shallow(y))
    coo_check(t_shallow(z), want, COO[out], (2 * m + 3, n + 2))


@pytest.mark.parametrize("m, n", SHAPES)
@pytest.mark.parametrize("kx", "dln")
@pytest.mark.parametrize("kv", "diln")
def test_rbind2_coo_vec_first_and_last(gpu, m, n, kx, kv):
    x, v = T(kx, m, n, 3, dup=True), V(kv, n + 4, 4, shuffle=True)
    out = kind_of(x, v)
    coo_check(mx.rbind2(x, v), coo_expected([x, v], [0, m], out), COO[out], (m + 1, n + 4))
    coo_check(mx.rbind2(v, x), coo_expected([x, v], [1, 0], out), COO[out], (m + 1, n + 4))      # R/rbind.R:497-498
    z = mx.cbind2(t_shallow(x), v)                                                               # R/cbind.R:26-28
    coo_check(t_shallow(z), coo_expected([x, v], [0, m], out), COO[out], (m + 1, n + 4))
    z = mx.cbind2(v, t_shallow(x))
    coo_check(t_shallow(z), coo_expected([x, v], [1, 0], out), COO[out], (m + 1, n + 4))


def test_rbind2_coo_with_csc_and_empty_vector(gpu):
    x, c = T("l", 10, 3, 5), Cm(10, 3, 6)
    got = mx.rbind2(x, c)                                                  # R/rbind.R:532-535
    assert type(got) is dgTMatrix and got.Dim == (20, 3)
    np.testing.assert_array_equal(dense(got), np.vstack([dense(x), dense(c)]))
    np.testing.assert_array_equal(dense(mx.rbind2(c, x)), np.vstack([dense(c), dense(x)]))
    e = nsparseVector(np.zeros(0, np.int32), None, 2)
    got = mx.rbind2(e, T("n", 10, 3, 7))
    assert type(got) is ngTMatrix and got.Dim == (11, 3) and got.i.min() >= 1


# ----------------------------------------------------------------------------------------------- CSR + vector column
def cbind_svec_expected(X, v, first, out):
    order = np.argsort(v.i, kind="stable")
    vi, vx = v.i[order], None if v.x is None else v.x[order]
    nrows = max(X.Dim[0], v.length)
    xv = convert(X.x, X.j.size, kind_of(X), out, False)
    vv = convert(vx, vi.size, letter(v), out, True)
    p, j, x = [0], [], []
    for r in range(nrows):
        s, e = (X.p[r], X.p[r + 1]) if r < X.Dim[0] else (X.p[-1], X.p[-1])
        cols, vals = list(X.j[s:e] + (1 if first else 0)), [] if xv is None else list(xv[s:e])
        k = np.flatnonzero(vi == r + 1)
        if k.size:
            cols = [0] + cols if first else cols + [X.Dim[1]]
            if vv is not None:
                vals = [vv[k[0]]] + vals if first else vals + [vv[k[0]]]
        j += cols
        x += vals
        p.append(len(j))
    return dict(indptr=np.array(p, np.int32), indices=np.array(j, np.int32),
                values=None if out == "n" else np.array(x, np.float64 if out == "d" else np.int32))


@pytest.mark.parametrize("m, n", SHAPES)
@pytest.mark.parametrize("kx", "dln")
@pytest.mark.parametrize("kv", "diln")
def test_cbind2_csr_svec(gpu, m, n, kx, kv):
    X = R(kx, m, n, 11, names=True)
    vectors = {"shorter": V(kv, m - 3, 12), "longer": V(kv, m + 5, 13), "empty": V(kv, m, 14, n=0),
               "past_the_end": SVEC[kv]([m + 2, m + 7], None if kv == "n" else np.ones(2), m + 7),
               "unsorted": V(kv, m, 15, n=min(m, 7), shuffle=True), "full": V(kv, m, 16, n=m)}
    for name, v in vectors.items():
        out = kind_of(X, v)
        for first in (False, True):
            want = cbind_svec_expected(X, v, first, out)
            got = mx.cbind2(v, X) if first else mx.cbind2(X, v)
            assert type(got) is CSR[out] and got.Dim == (max(m, v.length), n + 1), name
            same_csr(dict(indptr=got.p, indices=got.j, values=got.x), want)
            assert got.Dimnames[0][:m] == X.Dimnames[0] and len(got.Dimnames[0]) == got.Dim[0]
            assert got.Dimnames[1] == ([""] + X.Dimnames[1] if first else X.Dimnames[1] + [""])
            order = np.argsort(v.i, kind="stable")
            dev = dev_cbind_svec(("dln".index(kx), X.p, X.j, X.x, m), n, "dln".index(kx), v.i[order],
                                 None if v.x is None else v.x[order], 3 + "diln".index(kv), v.length, first,
                                 "dln".index(out))
            same_csr(dev, want)


# ----------------------------------------------------------------------------------------------- dense vectors
def dense_vectors(n, seed):
    rng = np.random.default_rng(seed)
    d = np.round(rng.normal(size=n), 1)
    d[::3], d[1::5] = 0.0, np.nan
    i = rng.integers(-2, 3, n).astype(np.int32)
    i[::4] = 0
    if n > 2:
        i[2] = NA
    l = mx.RLogical(np.where(rng.random(n) < 0.2, NA, rng.integers(0, 2, n)))
    return {"numeric": d, "integer": i, "logical": l, "bool": rng.random(n) < 0.5}


def as_double(v):
    a = np.asarray(v)
    if a.dtype == np.bool_:
        return a.astype(np.float64)
    if a.dtype == np.int32:
        return np.where(a == NA, np.nan, (a != 0).astype(np.float64) if getattr(v, "r_logical", False) else a.astype(np.float64))
    return a


def stored(out):
    """dense mask of the stored cells"""
    P = t_shallow(out) if isinstance(out, dgCMatrix) else out
    mask = np.zeros(P.Dim, bool)
    mask[np.repeat(np.arange(P.Dim[0]), np.diff(P.p)), P.j] = True
    return mask.T if isinstance(out, dgCMatrix) else mask


@pytest.mark.parametrize("m, n", SHAPES)
@pytest.mark.parametrize("fmt", ["R", "C"])
def test_dense_vectors_all_eight_orders(gpu, m, n, fmt):
    X = R("l", m, n, 21) if fmt == "R" else Cm(m, n, 22)
    cls = dgRMatrix if fmt == "R" else dgCMatrix
    DX = dense(X)
    for bind2, length, stack, axis in ((mx.rbind2, n, np.vstack, 0), (mx.cbind2, m, np.hstack, 1)):
        for name, v in list(dense_vectors(length, 23).items()) + [("recycled", np.array([2.5])), ("zero", np.zeros(1))]:
            full = np.repeat(as_double(v), length) if np.asarray(v).size == 1 else as_double(v)
            line = full.reshape(1, -1) if axis == 0 else full.reshape(-1, 1)
            for vec_first in (False, True):
                got = bind2(v, X) if vec_first else bind2(X, v)
                assert type(got) is cls, (name, vec_first)
                np.testing.assert_array_equal(dense(got), stack([line, DX] if vec_first else [DX, line]))
                where = stored(got)
                mine = (where[0, :] if vec_first else where[-1, :]) if axis == 0 else (where[:, 0] if vec_first else where[:, -1])
                np.testing.assert_array_equal(mine, full != 0)             # no stored entry comes from a zero; NA stays


@pytest.mark.parametrize("n", [0, 1, 4096, 4097, 9001])
def test_dense_to_svec(gpu, n):
    """the compaction across tiles (4096 cells each), exact"""
    for name, v in dense_vectors(n, 31).items():
        if name == "bool":
            continue
        dt = {"numeric": MX_F64, "integer": MX_I32, "logical": MX_LGL}[name]
        got = G.dense_to_svec(np.asarray(v), dt)
        a = as_double(v)
        keep = np.flatnonzero(a != 0)
        np.testing.assert_array_equal(got["ii"], (keep + 1).astype(np.int32))
        same_values(got["xx"], a[keep])


# ----------------------------------------------------------------------------------------------- rows, by dense equality
def rows_expected(ops):
    ncol = max(o.length if isinstance(o, mx.sparseVector) else o.Dim[1] for o in ops)
    return np.vstack([pad(np.atleast_2d(dense(o)), (1 if isinstance(o, mx.sparseVector) else o.Dim[0], ncol)) for o in ops])


@pytest.mark.parametrize("m, n", SHAPES)
def test_rbind2_row_forms(gpu, m, n):
    for kx in "dln":
        for ky in "dln":
            x, y = R(kx, m, n, 41), R(ky, m + 1, n + 2, 42)
            v, w = V(kx if kx != "d" else "i", n + 1, 43), V(ky, n, 44, shuffle=True)
            for a, b in ((x, y), (x, w), (v, y), (v, w), (T(kx, m, n, 45), y), (x, T(ky, m, n + 1, 46))):
                got = mx.rbind2(a, b)
                assert type(got) is CSR[kind_of(a, b)], (kx, ky)
                np.testing.assert_array_equal(dense(got), rows_expected([a, b]))
            named = R(kx, m, n, 41, names=True)
            got = mx.rbind2(named, w)
            assert got.Dimnames[0] == named.Dimnames[0] + [""] and got.Dimnames[1] == named.Dimnames[1]
    x, c = R("l", m, n, 47), Cm(m + 2, n, 48)
    for a, b in ((x, c), (c, x)):
        got = mx.rbind2(a, b)
        assert type(got) is dgRMatrix
        np.testing.assert_array_equal(dense(got), rows_expected([a, b]))
    got = mx.rbind2(c, Cm(m, n + 3, 49))                                  # R/rbind.R:279-280
    assert type(got) is dgCMatrix and got.Dim == (2 * m + 2, n + 3)
    np.testing.assert_array_equal(dense(got), np.vstack([pad(dense(c), (m + 2, n + 3)), dense(Cm(m, n + 3, 49))]))


@pytest.mark.parametrize("m, n", SHAPES)
def test_rbind_csr_and_the_folds(gpu, m, n):
    ops = [R("l", m, n, 51, names="rows"), V("d", n + 2, 52), R("n", 0, n + 9, 53), R("n", m, n, 54), V("n", n, 55),
           V("i", n, 56), np.arange(n, dtype=np.float64) % 3, V("l", n, 57, n=0)]
    got = mx.rbind_csr(*ops)
    assert type(got) is dgRMatrix and got.Dim == (2 * m + 5, n + 9)       # ncols counts the dropped rowless matrix
    live = [o for o in ops if not (isinstance(o, mx.RsparseMatrix) and o.Dim[0] == 0)]
    as_ops = [dsparseVector(np.flatnonzero(o) + 1, o[o != 0], o.size) if isinstance(o, np.ndarray) else o for o in live]
    np.testing.assert_array_equal(dense(got), pad(rows_expected(as_ops), (2 * m + 5, n + 9)))
    assert got.Dimnames == [ops[0].Dimnames[0] + [""] * (m + 5), None]    # R/rbind.R:99-111
    for kinds, want in (("lnl", lgRMatrix), ("nnn", ngRMatrix)):
        three = [R(kinds[0], m, n, 58), V(kinds[1], n, 59), R(kinds[2], 3, n, 60)]
        got = mx.rbind_csr(*three)
        assert type(got) is want
        np.testing.assert_array_equal(dense(got), rows_expected(three))
    one = mx.rbind_csr(V("l", n, 61))                                     # :60-61
    assert type(one) is lgRMatrix and one.Dim == (1, n)
    folded = mx.rbind(ops[0], ops[1], ops[3])
    np.testing.assert_array_equal(dense(folded), dense(mx.rbind_csr(ops[0], ops[1], ops[3])))
    folded = mx.cbind(ops[0], V("d", m, 62), R("d", m, 2, 63))
    assert type(folded) is dgRMatrix and folded.Dim == (m, n + 3)


@pytest.mark.parametrize("m, n", SHAPES)
def test_cbind_forms(gpu, m, n):
    for kx in "dln":
        for ky in "dln":
            x, y = R(kx, m, n, 71, names=True), R(ky, m + 4, 2, 72, names=True)
            for a, b in ((x, y), (y, x), (T(kx, m, n, 73), y), (x, T(ky, m - 2, 4, 74))):
                got = mx.cbind2(a, b)
                rows = max(a.Dim[0], b.Dim[0])
                assert type(got) is CSR[kind_of(a, b)] and got.Dim == (rows, a.Dim[1] + b.Dim[1])
                np.testing.assert_array_equal(dense(got), np.hstack([pad(dense(a), (rows, a.Dim[1])),
                                                                      pad(dense(b), (rows, b.Dim[1]))]))
            got = mx.cbind2(x, y)
            assert got.Dimnames == [x.Dimnames[0] + y.Dimnames[0][:4], x.Dimnames[1] + y.Dimnames[1]]
    c, c2, v, w = Cm(m, n, 75), Cm(m + 1, 2, 76), V("l", m, 77), V("n", m + 2, 78)
    for a, b in ((c, c2), (c, v), (w, c), (v, w)):
        got = mx.cbind2(a, b)
        assert type(got) is dgCMatrix
        cols = [dense(o).reshape(-1, 1) if isinstance(o, mx.sparseVector) else dense(o) for o in (a, b)]
        rows = max(k.shape[0] for k in cols)
        np.testing.assert_array_equal(dense(got), np.hstack([pad(k, (rows, k.shape[1])) for k in cols]))
    got = mx.cbind2(R("n", m, 0, 79), v)                                   # a matrix without columns: the vector alone
    assert type(got) is lgRMatrix and got.Dim == (m, 1)
    np.testing.assert_array_equal(dense(got)[:, 0], dense(v))


# ----------------------------------------------------------------------------------------------- the device forms
def to_dev(X):
    return D.DeviceCSR.from_host(X.p, X.j, X.x, X.Dim[1])


def host(A):
    p, j, x = A.to_host()
    return dict(indptr=p, indices=j, values=x)


def tt(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("m, n", SHAPES)
def test_device_forms_against_the_exports(gpu, m, n):
    ops = [R("l", m, n, 81), V("d", n + 2, 82), R("n", m, n, 83), V("i", n, 84), R("n", 0, n, 85), V("l", n, 86), V("n", n, 87)]
    for take, out_kind in ((slice(None), 0), ([0, 2, 5, 6], 1), ([2, 4, 6], 2)):
        sel = ops[take] if isinstance(take, slice) else [ops[k] for k in take]
        items = [to_dev(o) if isinstance(o, mx.RsparseMatrix) else (tt(o.i), tt(o.x), o.length, letter(o)) for o in sel]
        got = D.csr_rbind(items)
        objs = [("dln".index(kind_of(o)), o.p, o.j, o.x, o.Dim[0]) if isinstance(o, mx.RsparseMatrix)
                else (3 + "diln".index(letter(o)), None, o.i, o.x, 1) for o in sel]
        same_csr(host(got), G.concat_csr_batch(objs, out_kind))
        assert got.K == max(o.length if isinstance(o, mx.sparseVector) else o.Dim[1] for o in sel)
    for k in "dln":
        x, y = R(k, m, n, 88), R(k, m + 3, 4, 89)
        fn = {"d": G.cbind_csr_numeric, "l": G.cbind_csr_logical}.get(k)
        want = fn(x.p, x.j, x.x, y.p, y.j + n, y.x) if fn else G.cbind_csr_binary(x.p, x.j, y.p, y.j + n)
        got = host(D.csr_cbind(to_dev(x), to_dev(y)))
        np.testing.assert_array_equal(got["indptr"], want["indptr"])
        np.testing.assert_array_equal(got["indices"], want["indices"])
        if k != "n":
            same_values(got["values"], want["values"])
        for kv in "diln":
            v = V(kv, m + 2, 90)
            out = "dln".index(kind_of(x, v))
            for first in (False, True):
                want = G.cbind_csr_svec(x.p, x.j, x.x, n, "dln".index(k), v.i, v.x, 3 + "diln".index(kv), v.length, first, out)
                same_csr(host(D.csr_cbind_svec(to_dev(x), tt(v.i), tt(v.x), v.length, first, kind=kv)), want)
