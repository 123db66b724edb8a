"""The outer products of `%*%` with a one-column CSR and the float32 row vector x CSC product (outer.hip, DESIGN.md
§4.14), through matrixextra_amd.exports, against the reference's own compiled C++ (oracle/ref.py, where
oracle/_ref/libmxref.so exists) and against the numpy models below, which the same tests pin to the reference.

Known defect of the reference, not copied (as the scratch-overflow hazard in oracle/ref.py's docstring): matmul.cpp:808
reads y_values[col] where it means y_values[ix], an out-of-bounds read whenever y stores fewer positions than its
length.  The reference is therefore asked only about vectors that store every position (i = 1..length), where
y_values[col] is in bounds and equals y_values[k]; genuinely sparse vectors are checked against the model alone.
The reference also sizes the dense outer product as length(indices) * dim, a zero tail when a row stores more than one
entry: it is asked only about operands with at most one entry per row.

Row vector: the lane-group reduction reorders the float sum, so per column |got - ref| <= 2 * len * 2^-24 *
sum |a_i * v_i| (twice the standard bound of a length-len float32 sum, covering both orders); columns of length 0 or
1 are exactly equal."""
import ctypes as C

import numpy as np
import pytest

import devmem
from oracle import ref as Ref

NA_INT = np.int32(-2147483648)
NA_REAL = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
MS = [0, 1, 2, 63, 64, 65, 300]
DIMS = [0, 1, 63, 64, 65, 130]
PATTERNS = ["all_empty", "ends_empty", "none_empty", "mixed"]
SPECIAL = np.array([np.nan, np.inf, -np.inf, NA_REAL, -0.0, 0.0, 0.1, 1e-50, 1e300, -1e-200, -2.5, 16777217.0])
VSPECIAL = np.array([0.0, -0.0, np.nan, np.inf, 1e-200, -3.5, NA_REAL, 0.1])


def have_ref():
    return Ref.available()


def same(got, want, what):
    """== on values, NaN-aware (a NaN matches a NaN) and sign-of-zero-aware (the other bits must be equal)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), what
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.flatnonzero(got[~gn].view(bits) != want[~wn].view(bits))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first {got[~gn][bad[0]]!r} vs {want[~wn][bad[0]]!r}"


def same_triple(got, want, what):
    for k in ("indptr", "indices", "values"):
        same(got[k], want[k], f"{what}[{k}]")


def one_column(m, pattern, seed):
    """CSR triple of an m x 1 matrix with at most one entry per row; the values walk through SPECIAL"""
    rng = np.random.default_rng(seed)
    full = np.ones(m, dtype=bool)
    if pattern == "all_empty":
        full[:] = False
    elif pattern == "ends_empty" and m:
        full[0] = full[-1] = False
    elif pattern == "mixed":
        full = rng.random(m) < 0.5
    p = np.concatenate([[0], np.cumsum(full)]).astype(np.int32)
    n = int(p[-1])
    x = np.round(rng.normal(size=n), 3)
    x[:min(n, SPECIAL.size)] = SPECIAL[:min(n, SPECIAL.size)]
    if n > 20:
        x[rng.permutation(n)[:SPECIAL.size]] = SPECIAL
    return p, np.zeros(n, dtype=np.int32), x


def dense_vector(dim, seed):
    rng = np.random.default_rng(seed)
    v = np.round(rng.normal(size=dim), 3)
    k = min(dim, VSPECIAL.size)
    v[rng.permutation(dim)[:k]] = VSPECIAL[:k]
    return v


# ----------------------------------------------------------------------------- numpy models
def model_dense(colvec, p, x, f32):
    p = p.astype(np.int64)
    full = p[:-1] < p[1:]
    dim = colvec.size
    a = x[p[:-1][full]]
    with np.errstate(all="ignore"):
        if f32:
            vals = (np.float32(0) + a.astype(np.float32)[:, None] * colvec.astype(np.float32)[None, :]).astype(np.float64)
        else:
            vals = np.where(a[:, None] == 0, 0.0, 0.0 + a[:, None] * colvec[None, :])     # daxpy returns on alpha == 0
    return dict(indptr=np.concatenate([[0], np.cumsum(full * dim)]).astype(np.int32),
                indices=np.tile(np.arange(dim, dtype=np.int32), int(full.sum())), values=vals.reshape(-1))


def model_svec(p, x, yi, yv, length, kind):
    p = p.astype(np.int64)
    full = np.flatnonzero(p[:-1] < p[1:]).astype(np.int32)
    a = x[p[:-1][full]]
    counts = np.zeros(length + 1, dtype=np.int64)
    counts[yi] = full.size
    vals = []
    with np.errstate(all="ignore"):
        for k in range(yi.size):
            if kind == "binary":
                vals.append(a.copy())
            elif kind == "numeric":
                vals.append(yv[k] * a)
            else:
                vals.append(np.full(a.size, NA_REAL) if yv[k] == NA_INT else float(yv[k]) * a)
    return dict(indptr=np.cumsum(counts).astype(np.int32), indices=np.tile(full, yi.size),
                values=np.concatenate(vals) if vals else np.zeros(0))


def model_rowvec(v, p, i, x):
    out = np.zeros((1, p.size - 1), dtype=np.float32)
    for c in range(p.size - 1):
        acc = np.float32(0)
        for k in range(p[c], p[c + 1]):
            acc = np.float32(np.float64(acc) + x[k] * np.float64(v[i[k]])) if x is not None else np.float32(acc + v[i[k]])
        out[0, c] = acc
    return out


# ----------------------------------------------------------------------------- dense outer
@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_dense_outer_is_bit_exact(gpu, m, f32):
    from matrixextra_amd import exports as G
    name = "matmul_colvec_by_scolvecascsr" + ("_f32" if f32 else "")
    for dim in DIMS:
        for n, pattern in enumerate(PATTERNS):
            p, j, x = one_column(m, pattern, 100 * m + n)
            v = dense_vector(dim, 7 * dim + m)
            with np.errstate(invalid="ignore", over="ignore"):
                v = v.astype(np.float32) if f32 else v
            got = getattr(G, name)(v, p, j, x)
            what = f"{name} m={m} dim={dim} {pattern}"
            want = model_dense(v, p, x, f32)
            same_triple(got, want, what + " vs model")
            if have_ref():
                same_triple(want, getattr(Ref, name)(v, p, j, x), what + ": model vs reference")


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_dense_outer_signed_zero_and_narrowing(gpu, f32):
    """a negative value times 0.0 is +0 (axpy into a zeroed slot); a stored zero leaves zeros under daxpy's quick return
    and gives NaN against Inf in float; 0.1 and 16777217 are not representable in float; an underflowing negative
    product is +0, not -0"""
    from matrixextra_amd import exports as G
    p = np.arange(7, dtype=np.int32)
    x = np.array([-2.0, 0.0, 0.1, 16777217.0, -1e-200, -1e-30])
    v = np.array([0.0, np.inf, 3.0, 1e-200, 1e-30, -0.0])
    with np.errstate(invalid="ignore", over="ignore"):
        v = v.astype(np.float32) if f32 else v
    name = "matmul_colvec_by_scolvecascsr" + ("_f32" if f32 else "")
    got = getattr(G, name)(v, p, np.zeros(6, np.int32), x)
    vals = got["values"].reshape(6, 6)
    assert vals[0, 0] == 0.0 and not np.signbit(vals[0, 0]) and not np.signbit(vals[0, 5])
    assert np.isnan(vals[1, 1]) if f32 else (vals[1, 1] == 0.0 and not np.signbit(vals[1, 1]))
    assert vals[2, 2] == (float(np.float32(0.1) * np.float32(3.0)) if f32 else 0.1 * 3.0)
    assert vals[3, 2] == (16777216.0 * 3.0 if f32 else 16777217.0 * 3.0)
    assert vals[4, 3] == 0.0 and not np.signbit(vals[4, 3])
    assert vals[5, 4] == (0.0 if f32 else -1e-30 * 1e-30) and not (f32 and np.signbit(vals[5, 4]))
    same_triple(got, model_dense(v, p, x, f32), name + " vs model")
    if have_ref():
        same_triple(got, getattr(Ref, name)(v, p, np.zeros(6, np.int32), x), name + " vs reference")


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_dense_outer_row_with_two_entries(gpu, f32):
    """model only (the reference pads to length(indices) * dim): the first value is used, the length is out_indptr[m]"""
    from matrixextra_amd import exports as G
    p = np.array([0, 0, 2, 3, 3, 6], dtype=np.int32)
    x = np.array([2.0, 100.0, -1.5, 4.0, 200.0, 300.0])
    v = dense_vector(65, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = v.astype(np.float32) if f32 else v
    got = getattr(G, "matmul_colvec_by_scolvecascsr" + ("_f32" if f32 else ""))(v, p, np.zeros(6, np.int32), x)
    assert list(got["indptr"]) == [0, 0, 65, 130, 130, 195]
    assert got["indices"].size == got["values"].size == got["indptr"][-1] == 195
    same_triple(got, model_dense(v, p, x, f32), "two entries in a row")
    same(got["values"][130:], model_dense(v, np.array([0, 1], np.int32), np.array([4.0]), f32)["values"], "first value")


# ----------------------------------------------------------------------------- sparse outer
KINDS = ["numeric", "integer", "logical", "binary"]


def svec_values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "numeric":
        v = np.round(rng.normal(size=n), 3)
        k = min(n, VSPECIAL.size)
        v[rng.permutation(n)[:k]] = VSPECIAL[:k]
        return v
    if kind == "integer":
        v = rng.integers(-5, 6, size=n).astype(np.int32)
    elif kind == "logical":
        v = rng.integers(0, 2, size=n).astype(np.int32)
    else:
        return None
    v[rng.random(n) < 0.25] = NA_INT
    return v


def call_svec(mod, kind, p, j, x, yi, yv, length):
    fn = getattr(mod, "matmul_spcolvec_by_scolvecascsr_" + kind)
    return fn(p, j, x, yi, length) if kind == "binary" else fn(p, j, x, yi, yv, length)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", KINDS)
def test_sparse_outer_is_bit_exact(gpu, m, kind):
    from matrixextra_amd import exports as G
    for n, pattern in enumerate(PATTERNS):
        p, j, x = one_column(m, pattern, 100 * m + n)
        for length in (1, 70, 257):
            rng = np.random.default_rng(length + m)
            full = np.arange(1, length + 1, dtype=np.int32)
            inner = np.sort(rng.permutation(np.arange(2, length))[:length // 3]).astype(np.int32)
            ends = np.unique(np.array([1, length], dtype=np.int32))
            for label, yi in (("every", full), ("ends", np.unique(np.concatenate([ends, inner]))),
                              ("nothing", np.zeros(0, np.int32))):
                yv = svec_values(kind, yi.size, length + 3 * m)
                what = f"{kind} m={m} {pattern} length={length} {label}"
                got = call_svec(G, kind, p, j, x, yi, yv, length)
                want = model_svec(p, x, yi, yv, length, kind)
                same_triple(got, want, what + " vs model")
                if label == "every" and have_ref():         # y_values[col] is y_values[k] there (matmul.cpp:808)
                    same_triple(want, call_svec(Ref, kind, p, j, x, yi, yv, length), what + ": model vs reference")


@pytest.mark.gpu
def test_sparse_outer_more_than_one_chunk(gpu):
    """2500 non-empty rows: three chunks of 1024 compacted rows per stored position, the last one partial"""
    from matrixextra_amd import exports as G
    rng = np.random.default_rng(5)
    fullrows = rng.random(5000) < 0.5
    fullrows[np.flatnonzero(fullrows)[2500:]] = False
    p = np.concatenate([[0], np.cumsum(fullrows)]).astype(np.int32)
    assert p[-1] == 2500
    x = rng.normal(size=2500)
    yi = np.array([2, 3, 9], dtype=np.int32)
    yv = np.array([1.5, np.nan, -2.0])
    got = G.matmul_spcolvec_by_scolvecascsr_numeric(p, np.zeros(2500, np.int32), x, yi, yv, 9)
    same_triple(got, model_svec(p, x, yi, yv, 9, "numeric"), "chunks")


# ----------------------------------------------------------------------------- row vector
@pytest.fixture(scope="module")
def csc_operand():
    """300 rows; columns of length 0, 1, 64 and 300, three times over"""
    rng = np.random.default_rng(11)
    lens = np.array([0, 1, 64, 300] * 3)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    i = np.concatenate([np.sort(rng.permutation(300)[:n]) for n in lens]).astype(np.int32)
    x = rng.normal(size=i.size)
    v = rng.normal(size=300).astype(np.float32)
    return lens, p, i, x, v


@pytest.mark.gpu
@pytest.mark.parametrize("with_values", [True, False], ids=["values", "binary"])
def test_rowvec_by_csc(gpu, csc_operand, with_values):
    from matrixextra_amd import exports as G
    lens, p, i, x, v = csc_operand
    xs = x if with_values else None
    got = G.matmul_rowvec_by_csc(v, p, i, x) if with_values else G.matmul_rowvec_by_cscbin(v, p, i)
    assert got.dtype == np.float32 and got.shape == (1, lens.size)
    want = model_rowvec(v, p, i, xs)
    if have_ref():
        ref = Ref.matmul_rowvec_by_csc(v, p, i, x) if with_values else Ref.matmul_rowvec_by_cscbin(v, p, i)
        same(want, np.asarray(ref, dtype=np.float32).reshape(1, -1), "model vs reference")
    terms = np.abs((x if with_values else 1.0) * v[i].astype(np.float64))
    for c, n in enumerate(lens):
        bound = 2.0 * n * 2.0 ** -24 * terms[p[c]:p[c + 1]].sum()
        err = abs(float(got[0, c]) - float(want[0, c]))
        print(f"column {c} (len {n}): |got - ref| = {err:.3e}, bound {bound:.3e}")
        if n <= 1:
            assert got[0, c] == want[0, c]
        else:
            assert err <= bound


@pytest.mark.gpu
def test_rowvec_refuses_an_index_outside_the_vector(gpu):
    from matrixextra_amd import _lib, exports as G
    with pytest.raises(_lib.MxError, match="outside the vector"):
        G.matmul_rowvec_by_cscbin(np.ones(3, np.float32), np.array([0, 1], np.int32), np.array([3], np.int32))


# ----------------------------------------------------------------------------- overflow
@pytest.mark.gpu
def test_overflow_is_refused_before_anything_is_allocated(gpu):
    import torch
    from matrixextra_amd import _lib, exports as G
    p = np.arange(70001, dtype=np.int32)                   # 70 000 non-empty rows x 40 000 > INT32_MAX
    j, x = np.zeros(70000, np.int32), np.ones(70000)
    assert p.nbytes + x.nbytes < 2 ** 20
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.MxError, match="int32 index range"):
        G.matmul_colvec_by_scolvecascsr(np.ones(40000), p, j, x)
    with pytest.raises(_lib.MxError, match="int32 index range"):
        G.matmul_colvec_by_scolvecascsr_f32(np.ones(40000, np.float32), p, j, x)
    with pytest.raises(_lib.MxError, match="int32 index range"):
        G.matmul_spcolvec_by_scolvecascsr_numeric(p, j, x, np.arange(1, 40001, dtype=np.int32), np.ones(40000), 40000)
    with pytest.raises(_lib.MxError, match="int32 index range"):
        G.matmul_spcolvec_by_scolvecascsr_binary(p, j, x, np.arange(1, 40001, dtype=np.int32), 40000)
    assert torch.cuda.memory_allocated() == before


# ----------------------------------------------------------------------------- guarded buffers
@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_dense_outer_in_guarded_buffers(gpu, f32):
    lib = gpu.load()
    p, j, x = one_column(300, "mixed", 1)
    p = p.copy()
    x = np.concatenate([x, [9.0]])                          # the last row stores two entries
    j = np.zeros(x.size, np.int32)
    p[-1] += 1
    v = dense_vector(65, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        v = v.astype(np.float32) if f32 else v
    A = devmem.GCsr(p, j, x)
    gv = devmem.GuardedVec(v.dtype, data=v)
    gws = devmem.GuardedVec(np.uint8, n=lib.mxd_csr_outer_dense_workspace_bytes(A.m))
    gp = devmem.GuardedVec(np.int32, n=A.m + 1)
    total = C.c_int64(-1)
    gpu.check(lib.mxd_csr_outer_dense_count(A.m, v.size, A.p.ptr, gws.ptr, gp.ptr, C.byref(total), None))
    want = model_dense(v, p, x, f32)
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    assert nout == want["indptr"][-1] == indptr[-1]
    gj, gx = devmem.GuardedVec(np.int32, n=nout + devmem.SLACK), devmem.GuardedVec(np.float64, n=nout + devmem.SLACK)
    gpu.check(lib.mxd_csr_outer_dense_fill(A.m, v.size, A.nnz, A.p.ptr, A.xptr, gv.ptr, gpu.MX_F32 if f32 else gpu.MX_F64,
                                           gp.ptr, gj.ptr, gx.ptr, None))
    devmem._sync()
    assert devmem.last_row_launch() == ("mxd_csr_outer_dense_fill", 64)
    devmem._untouched(A, gv)
    same_triple(dict(indptr=gp.result(), indices=gj.result(nout), values=gx.result(nout)), want, "guarded dense outer")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["numeric", "logical", "binary"])
def test_sparse_outer_in_guarded_buffers(gpu, kind):
    lib = gpu.load()
    p, j, x = one_column(300, "mixed", 4)
    length = 70
    yi = np.array([1, 2, 33, 64, 65, 70], dtype=np.int32)
    yv = svec_values(kind, yi.size, 8)
    dt = {"numeric": gpu.MX_F64, "logical": gpu.MX_LGL, "binary": gpu.MX_NONE}[kind]
    A = devmem.GCsr(p, j, x)
    gyi = devmem.GuardedVec(np.int32, data=yi)
    gyv = None if yv is None else devmem.GuardedVec(yv.dtype, data=yv)
    gws = devmem.GuardedVec(np.uint8, n=lib.mxd_csr_outer_svec_workspace_bytes(A.m, length))
    gp = devmem.GuardedVec(np.int32, n=length + 1)
    nonempty, total = C.c_int64(-1), C.c_int64(-1)
    gpu.check(lib.mxd_csr_outer_svec_count(A.m, A.nnz, A.p.ptr, A.xptr, gyi.ptr, yi.size, length, gws.ptr, gp.ptr,
                                           C.byref(nonempty), C.byref(total), None))
    want = model_svec(p, x, yi, yv, length, kind)
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    assert nonempty.value == p[-1] and nout == want["indptr"][-1] == indptr[-1]
    gi, gx = devmem.GuardedVec(np.int32, n=nout + devmem.SLACK), devmem.GuardedVec(np.float64, n=nout + devmem.SLACK)
    gpu.check(lib.mxd_csr_outer_svec_fill(A.m, gyi.ptr, yi.size, None if gyv is None else gyv.ptr, dt, length,
                                          nonempty.value, gws.ptr, gp.ptr, gi.ptr, gx.ptr, None))
    devmem._sync()
    devmem._untouched(A, gyi, gyv)
    gws._download()
    same_triple(dict(indptr=gp.result(), indices=gi.result(nout), values=gx.result(nout)), want, "guarded sparse outer")
