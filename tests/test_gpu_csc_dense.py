"""CSC * dense on the device: the nine multiply_csc_by_dense_* / logicaland_csc_by_dense_ignore_NAs exports (svec.hip's
csr_by_dense_kernel with CSC addressing; cscdense.hip's count / scan / fill), `dgCMatrix * matrix` in both orders and
both option settings, and device.csc_by_dense.

Expected results come from a numpy restatement of DESIGN.md §4.10's semantics table:

    keep NAs (default)   output column c = its stored rows (a repeated row once, with the first entry's value) with
                         x (op) d, plus every row whose dense cell is NA (f64 / float32: any NaN; integer / logical:
                         NA_INTEGER) and is not stored, with value NA_real_; rows ascending
    ignore NAs           values only: x (op) d for every entry in storage order; p is e1's own object, i a copy
    x (op) d             f64 / float32: x * d (float32 widened), NaN propagates; integer / logical: NA -> NA_real_,
                         else x * d (logical: x * (d != 0)); `&`: R's three-valued AND of R logicals

Values are compared bit for bit (uint64 view), so NA_real_ and other NaN payloads stay distinct; where x and d are
both NaN only NaN-ness is compared (which operand's payload survives is the hardware's choice).
"""
import numpy as np
import pytest
import torch

import matrixextra_amd as mx
from matrixextra_amd import exports as G
from conftest import rand_csr

pytestmark = pytest.mark.gpu

NA = np.int32(-2147483648)
NA_REAL = mx.NA_REAL
OTHER_NAN = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0]
F32_NAN = np.frombuffer(np.uint32(0x7FC00123).tobytes(), dtype=np.float32)[0]
KINDS = ("numeric", "float32", "integer", "logical")


def ignore_fn(kind):
    return getattr(G, "multiply_csc_by_dense_ignore_NAs_" + kind)


def keep_fn(kind):
    return getattr(G, "multiply_csc_by_dense_keep_NAs_" + kind)


@pytest.fixture
def opts():
    saved = dict(mx.options)
    yield mx.options
    mx.options.clear()
    mx.options.update(saved)


# ---------------------------------------------------------------------------------------------- restatement
def is_na(kind, d):
    return np.isnan(d) if kind in ("numeric", "float32") else d == NA


def op(kind, x, d):
    with np.errstate(all="ignore"):
        if kind == "numeric":
            return x * d
        if kind == "float32":
            return x * d.astype(np.float64)
        dd = d.astype(np.float64) if kind == "integer" else (d != 0).astype(np.float64)
        return np.where(d == NA, NA_REAL, x * dd)


def r_and(x, d):
    false = (x == 0) | (d == 0)
    na = (x == NA) | (d == NA)
    return np.where(false, 0, np.where(na, NA, 1)).astype(np.int32)


def flat_of(p, i, m):
    cols = np.repeat(np.arange(p.size - 1, dtype=np.int64), np.diff(p))
    return cols * m + i.astype(np.int64)


def ref_ignore(kind, p, i, x, D):
    d = np.asarray(D).reshape(-1, order="F")[flat_of(p, i, D.shape[0])]
    if kind == "and":
        return r_and(x, d), None
    both = (np.isnan(x) & np.isnan(d)) if kind in ("numeric", "float32") else None
    return op(kind, x, d), both


def ref_keep(kind, p, i, x, D):
    """(indptr, indices, values, both-NaN mask) of the NA-keeping product of a column-sorted CSC."""
    m, n = D.shape
    if m == 0 or n == 0:
        return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0, bool)
    f = flat_of(p, i, m)
    first = np.ones(f.size, bool)
    first[1:] = f[1:] != f[:-1]
    fs, xs = f[first], x[first]
    Df = np.asarray(D).reshape(-1, order="F")
    u = np.union1d(fs, np.flatnonzero(is_na(kind, Df)))
    vals = np.full(u.size, NA_REAL)
    pos = np.searchsorted(u, fs)
    vals[pos] = op(kind, xs, Df[fs])
    both = np.zeros(u.size, bool)
    if kind in ("numeric", "float32"):
        both[pos] = np.isnan(xs) & np.isnan(Df[fs])
    indptr = np.searchsorted(u, np.arange(n + 1, dtype=np.int64) * m).astype(np.int32)
    return indptr, (u % m).astype(np.int32), vals, both


def same_bits(got, want, both=None, msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    if got.dtype != np.float64:
        np.testing.assert_array_equal(got, want, err_msg=msg)
        return
    g, w = got.view(np.uint64).copy(), want.view(np.uint64).copy()
    if both is not None and both.any():
        assert np.isnan(got[both]).all(), msg
        g[both] = w[both] = 0
    np.testing.assert_array_equal(g, w, err_msg=msg)


def check_keep(kind, p, i, x, D, msg=""):
    got = keep_fn(kind)(p, i, x, D)
    ep, ei, ev, both = ref_keep(kind, p, i, x, D)
    np.testing.assert_array_equal(got["indptr"], ep, err_msg=msg)
    np.testing.assert_array_equal(got["indices"], ei, err_msg=msg)
    same_bits(got["values"], ev, both, msg)
    return got


def check_ignore(kind, p, i, x, D, msg=""):
    fn = G.logicaland_csc_by_dense_ignore_NAs if kind == "and" else ignore_fn(kind)
    want, both = ref_ignore(kind, p, i, x, D)
    same_bits(fn(p, i, x, D), want, both, msg)


def dense_of(kind, m, n, rng, na_frac=0.1):
    r = rng.random((m, n))
    if kind == "numeric":
        D = np.round(rng.normal(size=(m, n)), 2)
        D[r < na_frac / 2] = NA_REAL
        D[(r >= na_frac / 2) & (r < na_frac)] = OTHER_NAN
        D[(r >= na_frac) & (r < na_frac + 0.02)] = np.inf
        D[(r >= na_frac + 0.02) & (r < na_frac + 0.05)] = 0.0
    elif kind == "float32":
        D = np.round(rng.normal(size=(m, n)), 2).astype(np.float32)
        D[r < na_frac / 2] = np.float32(np.nan)
        D[(r >= na_frac / 2) & (r < na_frac)] = F32_NAN
        D[(r >= na_frac) & (r < na_frac + 0.02)] = np.float32(np.inf)
    elif kind == "integer":
        D = rng.integers(-5, 6, size=(m, n)).astype(np.int32)
        D[r < na_frac] = NA
    else:
        D = rng.integers(0, 2, size=(m, n)).astype(np.int32)
        D[r < na_frac] = NA
    return np.asfortranarray(D)


def csc_case(m, n, density, seed, stored_na=0.1):
    """CSC arrays (the CSR of X^T) with sorted rows; some stored values NA_real_ / another NaN / 0 / Inf."""
    p, i, x = rand_csr(n, m, density, seed)
    rng = np.random.default_rng(seed + 100)
    r = rng.random(x.size)
    x[r < stored_na / 2] = NA_REAL
    x[(r >= stored_na / 2) & (r < stored_na)] = OTHER_NAN
    x[(r >= stored_na) & (r < stored_na + 0.03)] = np.inf
    return p, i, x


def csc_to_dense(C):
    out = np.zeros(C.Dim)
    for c in range(C.Dim[1]):
        out[C.i[C.p[c]:C.p[c + 1]], c] = C.x[C.p[c]:C.p[c + 1]]
    return out


def dense_to_csc(A):
    A = np.asarray(A, dtype=np.float64)
    mask = (A != 0) | np.isnan(A)
    p = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int32)
    cc, rr = np.nonzero(mask.T)                           # column-major order: (column, row) pairs
    return mx.dgCMatrix(p, rr.astype(np.int32), A[rr, cc], A.shape)


# ---------------------------------------------------------------------------------------------- reference answers
def test_reference_csc_and_dense(gpu, opts):
    """test-operators.R "CSC and dense" (`*` cases), restated."""
    Dense = np.arange(1, 11, dtype=np.int32).reshape(5, 2, order="F")
    S = np.array([[0, 11], [0, 12], [1, 13], [2, 14], [3, 15]], dtype=np.float64)
    C = dense_to_csc(S)
    for ign in (False, True):
        opts["MatrixExtra.ignore_na"] = ign
        for r in (C * Dense, Dense * C):
            assert isinstance(r, mx.dgCMatrix)
            np.testing.assert_array_equal(csc_to_dense(r), Dense * S)
    DenseNew = Dense.astype(np.float64)
    DenseNew[0, 0] = NA_REAL
    opts["MatrixExtra.ignore_na"] = True                  # set_new_matrix_behavior
    for r in (DenseNew * C, C * DenseNew):
        assert isinstance(r, mx.dgCMatrix)
        np.testing.assert_array_equal(csc_to_dense(r), Dense * S)
    opts["MatrixExtra.ignore_na"] = False                 # restore_old_matrix_behavior
    for r in (DenseNew * C, C * DenseNew):
        assert isinstance(r, mx.dgCMatrix)
        np.testing.assert_array_equal(csc_to_dense(r), DenseNew * S)     # NaN == NaN here
        assert r.x[0].view(np.uint64) == NA_REAL.view(np.uint64)       # the new NA entry is NA_real_


def test_reference_nas_in_multiplication(gpu, opts):
    """test-operators.R "NAs in multiplication and ampersand", the CSC run of its `*` checks, restated."""
    Dense = np.arange(1, 11, dtype=np.int32).reshape(5, 2, order="F")
    DenseNew = Dense.astype(np.float64)
    DenseNew[0, 0] = NA_REAL
    DenseNew[1, 1] = 0
    DenseNew[2, 1] = 0
    DenseNew[4, 1] = NA_REAL
    S = np.array([[0, 11], [0, 12], [1, 13], [2, 14], [3, 15]], dtype=np.float64)
    S[1, 1] = S[3, 1] = S[4, 1] = NA_REAL
    C = dense_to_csc(S)
    DenseFilled = np.where(np.isnan(DenseNew), 0, DenseNew)
    SparseFilled = S.copy()
    SparseFilled[np.isnan(DenseNew) & ~np.isnan(SparseFilled)] = 0
    opts["MatrixExtra.ignore_na"] = True
    for r in (DenseNew * C, C * DenseNew):
        assert isinstance(r, mx.dgCMatrix)
        np.testing.assert_array_equal(csc_to_dense(r), DenseFilled * SparseFilled)
    opts["MatrixExtra.ignore_na"] = False
    for r in (DenseNew * C, C * DenseNew):
        assert isinstance(r, mx.dgCMatrix)
        np.testing.assert_array_equal(csc_to_dense(r), DenseNew * S)


# ---------------------------------------------------------------------------------------------- every export
@pytest.mark.parametrize("kind", KINDS)
def test_every_export_and_path(gpu, kind):
    for m, n, dens, na in ((37, 23, 0.2, 0.1), (130, 70, 0.05, 0.02), (300, 41, 0.5, 0.3), (64, 64, 0.1, 0.0)):
        p, i, x = csc_case(m, n, dens, seed=m + n)
        D = dense_of(kind, m, n, np.random.default_rng(m * n), na)
        msg = f"{kind} {m}x{n}"
        check_ignore(kind, p, i, x, D, msg)
        got = check_keep(kind, p, i, x, D, msg)
        if na == 0.0:                                     # no NA cell: the structure is the input's
            np.testing.assert_array_equal(got["indptr"], p)
            np.testing.assert_array_equal(got["indices"], i)


def test_keep_with_na_cells_only_inside_the_pattern(gpu):
    """NA cells that all lie on stored entries: no entry is added (the values-only route of the keep path)."""
    p, i, x = csc_case(50, 30, 0.2, seed=3)
    for kind in KINDS:
        D = dense_of(kind, 50, 30, np.random.default_rng(4), 0.0)
        cells = np.flatnonzero(np.random.default_rng(5).random(i.size) < 0.3)
        f = flat_of(p, i, 50)[cells]
        Df = D.reshape(-1, order="F").copy()
        Df[f] = NA_REAL if kind == "numeric" else F32_NAN if kind == "float32" else NA
        D = np.asfortranarray(Df.reshape(50, 30, order="F"))
        got = check_keep(kind, p, i, x, D, kind)
        np.testing.assert_array_equal(got["indices"], i)


def test_logicaland_ignore(gpu):
    rng = np.random.default_rng(11)
    for m, n in ((37, 23), (4097, 3), (1, 5000)):
        p, i, _ = rand_csr(n, m, 0.2, seed=m)
        xl = rng.choice(np.array([0, 1, NA], np.int32), size=i.size)
        D = dense_of("logical", m, n, rng, 0.2)
        check_ignore("and", p, i, xl, D, f"{m}x{n}")


def test_logical_dense_from_bool(gpu):
    p, i, x = csc_case(40, 30, 0.2, seed=6)
    B = np.random.default_rng(7).random((40, 30)) < 0.5
    want = ref_keep("logical", p, i, x, B.astype(np.int32))
    got = G.multiply_csc_by_dense_keep_NAs_logical(p, i, x, B)
    np.testing.assert_array_equal(got["indices"], want[1])
    same_bits(got["values"], want[2], want[3])


# ---------------------------------------------------------------------------------------------- edge shapes
EDGE = [  # (m, n, density, na_frac)
    (0, 3, 0.0, 0.0), (3, 0, 0.0, 0.0), (5, 4, 0.0, 0.3), (1, 1, 1.0, 0.0), (1, 1, 0.0, 1.0), (1, 7, 0.5, 0.3),
    (7, 1, 0.5, 0.3), (1, 200_000, 0.01, 0.01), (200_000, 1, 0.01, 0.01), (4096, 1, 0.1, 0.1), (4097, 1, 0.1, 0.1),
    (4095, 2, 0.1, 0.1), (64, 64, 0.1, 0.1), (64, 65, 0.1, 0.1), (1, 4097, 0.3, 0.2), (8193, 3, 0.05, 0.05),
    (63, 65, 0.3, 0.5),
]


@pytest.mark.parametrize("m,n,density,na", EDGE, ids=[f"{e[0]}x{e[1]}" for e in EDGE])
def test_edge_shapes(gpu, m, n, density, na):
    p, i, x = csc_case(m, n, density, seed=17) if n else (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for kind in ("numeric", "integer"):
        D = dense_of(kind, m, n, np.random.default_rng(18), na)
        check_keep(kind, p, i, x, D, f"{kind} {m}x{n}")
        check_ignore(kind, p, i, x, D, f"{kind} {m}x{n}")


def test_all_na_column_next_to_empty_columns(gpu):
    m, n = 300, 6
    p = np.array([0, 0, 0, 2, 2, 2, 3], np.int32)        # columns 0, 1, 3, 4 empty
    i = np.array([5, 299, 0], np.int32)
    x = np.array([2.0, NA_REAL, 4.0])
    D = np.ones((m, n))
    D[:, 1] = NA_REAL                                     # an all-NA empty column
    D[:, 2] = OTHER_NAN                                   # an all-NaN column with two stored rows
    D[7, 4] = np.nan
    D = np.asfortranarray(D)
    got = check_keep("numeric", p, i, x, D)
    np.testing.assert_array_equal(np.diff(got["indptr"]), [0, m, m, 0, 1, 1])
    assert got["values"][m + 5].view(np.uint64) == OTHER_NAN.view(np.uint64)   # 2 * NaN keeps the payload


def test_nnz_zero_with_na_cells(gpu):
    p = np.zeros(5, np.int32)
    D = np.asfortranarray(np.where(np.random.default_rng(1).random((9, 4)) < 0.4, NA, 3).astype(np.int32))
    got = check_keep("integer", p, np.zeros(0, np.int32), np.zeros(0), D)
    assert got["indices"].size == int((D == NA).sum())


# ---------------------------------------------------------------------------------------------- input handling
def test_repeated_rows_keep_the_first(gpu, opts):
    """a sorted column with a repeated row: one output entry, with the first entry's value (lower_bound skip)."""
    p = np.array([0, 3, 5], np.int32)
    i = np.array([1, 1, 2, 0, 0], np.int32)
    x = np.array([10.0, 20.0, 30.0, 5.0, 6.0])
    D = np.asfortranarray(np.array([[1.0, 2.0], [3.0, NA_REAL], [4.0, 5.0]]))
    got = check_keep("numeric", p, i, x, D)
    np.testing.assert_array_equal(got["indptr"], [0, 2, 4])
    np.testing.assert_array_equal(got["indices"], [1, 2, 0, 1])
    np.testing.assert_array_equal(got["values"][:3], [30.0, 120.0, 10.0])
    C = mx.dgCMatrix(p, i, x, (3, 2))
    r = C * D                                             # the stable sort keeps the order of the repeats
    np.testing.assert_array_equal(r.p, got["indptr"])
    np.testing.assert_array_equal(r.x[:3], [30.0, 120.0, 10.0])
    opts["MatrixExtra.ignore_na"] = True                  # values only: the repeats stay
    r = C * D
    np.testing.assert_array_equal(r.x, [30.0, 60.0, 120.0, 10.0, 12.0])


def test_unsorted_input_and_inplace_sort(gpu, opts):
    m, n = 60, 25
    p, i, x = csc_case(m, n, 0.3, seed=21)
    rng = np.random.default_rng(22)
    iu, xu = i.copy(), x.copy()
    for c in range(n):
        s, e = p[c], p[c + 1]
        perm = s + rng.permutation(e - s)
        iu[s:e], xu[s:e] = i[perm], x[perm]
    D = dense_of("numeric", m, n, rng, 0.1)
    ep, ei, ev, both = ref_keep("numeric", p, i, x, D)
    C = mx.dgCMatrix(p, iu.copy(), xu.copy(), (m, n))
    for r in (C * D, D * C):
        np.testing.assert_array_equal(r.p, ep)
        np.testing.assert_array_equal(r.i, ei)
        same_bits(r.x, ev, both)
    np.testing.assert_array_equal(C.i, iu)                # the caller's arrays stay untouched
    same_bits(C.x, xu)
    opts["MatrixExtra.inplace_sort"] = True
    r = C * D
    np.testing.assert_array_equal(r.i, ei)
    np.testing.assert_array_equal(C.i, i)                 # ... unless inplace_sort: sorted in place
    same_bits(C.x, x)


def test_values_only_shares_p_and_copies_i(gpu, opts):
    p, i, x = csc_case(40, 20, 0.3, seed=31)
    C = mx.dgCMatrix(p, i, x, (40, 20), [None, [f"c{k}" for k in range(20)]])
    D = dense_of("integer", 40, 20, np.random.default_rng(32), 0.2)
    opts["MatrixExtra.ignore_na"] = True
    r = C * D
    assert isinstance(r, mx.dgCMatrix) and r.Dim == C.Dim and r.Dimnames == C.Dimnames
    assert r.p is C.p and r.i is not C.i
    np.testing.assert_array_equal(r.i, C.i)
    want, _ = ref_ignore("integer", p, i, x, D)
    same_bits(r.x, want)


def test_float32_operands(gpu, opts):
    p, i, x = csc_case(30, 1, 0.4, seed=41)
    C = mx.dgCMatrix(p, i, x, (30, 1))
    v = np.round(np.random.default_rng(42).normal(size=30), 2).astype(np.float32)
    v[3] = F32_NAN
    for e2 in (mx.float32(v), mx.float32(v.reshape(30, 1))):   # a vector of nrow entries, recycled to one column
        for r in (C * e2, e2 * C):
            ep, ei, ev, both = ref_keep("float32", p, i, x, v.reshape(30, 1))
            np.testing.assert_array_equal(r.i, ei)
            same_bits(r.x, ev, both)


# ---------------------------------------------------------------------------------------------- large case
def test_large_20000_by_2000(gpu):
    m, n = 20_000, 2_000
    rng = np.random.default_rng(51)
    per_col = 200                                         # 1 % of the cells stored, 400 000 entries
    i = np.sort(np.stack([rng.choice(m, per_col, replace=False) for _ in range(n)]), axis=1).reshape(-1)
    i = i.astype(np.int32)
    p = np.arange(0, (n + 1) * per_col, per_col, dtype=np.int32)
    x = np.round(rng.normal(size=i.size), 3)
    D = np.asfortranarray(np.round(rng.normal(size=(m, n)), 3))
    D.reshape(-1, order="F")[rng.choice(m * n, m * n // 1000, replace=False)] = NA_REAL   # 0.1 % NA cells
    assert np.isnan(D).sum() == m * n // 1000
    check_keep("numeric", p, i, x, D, "large keep")
    check_ignore("numeric", p, i, x, D, "large ignore")
    r = D * mx.dgCMatrix(p, i, x, (m, n))
    ep, ei, ev, both = ref_keep("numeric", p, i, x, D)
    np.testing.assert_array_equal(r.p, ep)
    np.testing.assert_array_equal(r.i, ei)
    same_bits(r.x, ev, both)


# ---------------------------------------------------------------------------------------------- tensor API
def test_device_csc_by_dense(gpu):
    from matrixextra_amd import device as Dv
    m, n = 3000, 70
    p, i, x = csc_case(m, n, 0.05, seed=61)
    A = Dv.DeviceCSR.from_host(p, i, x, m)
    for kind, tdt in (("numeric", torch.float64), ("float32", torch.float32), ("integer", torch.int32),
                      ("logical", torch.bool)):
        Dh = dense_of(kind, m, n, np.random.default_rng(62), 0.05)
        if kind == "logical":
            Dh = np.random.default_rng(63).random((m, n)) < 0.5
        Dt = torch.from_numpy(np.ascontiguousarray(Dh)).to("cuda")          # row-major: strides are handled
        assert Dt.dtype == tdt
        ref_d = Dh.astype(np.int32) if kind == "logical" else Dh
        op_, oi, ox = Dv.csc_by_dense(A, Dt, keep_na=True)
        ep, ei, ev, both = ref_keep(kind, p, i, x, ref_d)
        np.testing.assert_array_equal(op_.cpu().numpy(), ep, err_msg=kind)
        np.testing.assert_array_equal(oi.cpu().numpy(), ei, err_msg=kind)
        same_bits(ox.cpu().numpy(), ev, both, kind)
        vp, vi, vx = Dv.csc_by_dense(A, Dt, keep_na=False)
        assert vp is A.indptr and vi.data_ptr() != A.indices.data_ptr()
        want, both = ref_ignore(kind, p, i, x, ref_d)
        same_bits(vx.cpu().numpy(), want, both, kind)
    Di = torch.from_numpy(np.where(np.random.default_rng(64).random((m, n)) < 0.1, NA, 1).astype(np.int32)).cuda()
    op_, oi, ox = Dv.csc_by_dense(A, Di, keep_na=True, logical=True)
    ep, ei, ev, both = ref_keep("logical", p, i, x, Di.cpu().numpy())
    np.testing.assert_array_equal(oi.cpu().numpy(), ei)
    same_bits(ox.cpu().numpy(), ev, both)
