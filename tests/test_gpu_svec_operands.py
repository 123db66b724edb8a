"""sparseVector operands on the device: sort_vector_indices_* (the radix sort of one segment), `X * v` / `v * X`
(svecmul.hip's count / scan / fill behind multiply_csr_by_svec_{no,keep}_NAs and device.csr_by_svec) and `X %*% v`.

Expected products come from a numpy restatement of DESIGN.md §4.11's row-class table.  With t = r mod length(v):

    t not stored, ignore NAs                          no entries
    t not stored, keep NAs                            the row's NaN / +-Inf entries in place order; a NaN unchanged,
                                                      +-Inf as the default NaN
    t stored, val finite (or ignore NAs, or no @x)    the whole row, x * val (copied without @x)
    t stored, val NaN / +-Inf, keep NAs, with @x      columns 0..ncol-1: NaN val everywhere, or for +-Inf the default
                                                      NaN with val * x at the stored columns

Values are compared bit for bit (uint64 view).  Where both factors of a product are NaN only NaN-ness is compared
(which payload survives is the hardware's choice); every test asserts that this covers at most 5 % of its entries.
The generators keep the restatement away from what the IEEE rules leave open: NaN / Inf values of v sit on rows whose
X values are finite (one dedicated case apart), and +-Inf never meets 0 (the sign of that NaN differs between hosts
and the device), so X has no stored zero and its Inf entries avoid rows whose vector value is 0.
"""
import numpy as np
import pytest
import torch

import matrixextra_amd as mx
from matrixextra_amd import device as Dv, exports as G

pytestmark = pytest.mark.gpu

NA = np.int32(-2147483648)
NA_REAL = mx.NA_REAL
OTHER_NAN = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0]
KINDS = ("numeric", "integer", "logical", "binary")
CLS = dict(numeric=mx.dsparseVector, integer=mx.isparseVector, logical=mx.lsparseVector, binary=mx.nsparseVector)
SPECIALS = dict(finite=[], na=[NA_REAL], nan=[OTHER_NAN], pinf=[np.inf], ninf=[-np.inf],
                mixed=[NA_REAL, OTHER_NAN, np.inf, -np.inf])


@pytest.fixture
def opts():
    saved = dict(mx.options)
    yield mx.options
    mx.options.clear()
    mx.options.update(saved)


# ---------------------------------------------------------------------------------------------- restatement
def as_f64(kind, vx):
    """@x of the vector as the kernel sees it (as.sparse.vector, R/operators.R:1601): f64, NA -> NA_real_; none."""
    if kind == "binary":
        return None
    if kind == "numeric":
        return vx
    return np.where(vx == NA, NA_REAL, vx.astype(np.float64))


def ref_mul(p, j, x, vi, vx, L, ncol, keep):
    """(indptr, indices, values, both-NaN mask) for a row-sorted X and a sorted v (vx f64 or None)."""
    m = p.size - 1
    pos = np.full(L, -1)
    pos[vi - 1] = np.arange(vi.size)
    cnt, J, V, B = np.zeros(m + 1, np.int64), [], [], []
    for r in range(m):
        s, e = p[r], p[r + 1]
        jr, xr = j[s:e], x[s:e]
        k = pos[r % L]
        if k < 0:
            if not keep:
                continue
            nf = ~np.isfinite(xr)
            jo, vo, bo = jr[nf], np.where(np.isinf(xr[nf]), np.nan, xr[nf]), np.zeros(int(nf.sum()), bool)
        elif vx is not None and keep and not np.isfinite(vx[k]):
            jo = np.arange(ncol, dtype=np.int32)
            if np.isnan(vx[k]):
                vo = np.full(ncol, vx[k])
            else:
                vo = np.full(ncol, np.nan)
                with np.errstate(all="ignore"):
                    vo[jr] = vx[k] * xr
            bo = np.zeros(ncol, bool)
        else:
            with np.errstate(all="ignore"):
                jo, vo = jr, (xr.copy() if vx is None else xr * vx[k])
            bo = np.zeros(jr.size, bool) if vx is None else np.isnan(xr) & np.isnan(vx[k])
        cnt[r + 1] = jo.size
        J.append(jo), V.append(vo), B.append(bo)
    cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt)          # noqa: E731
    return np.cumsum(cnt).astype(np.int32), cat(J, np.int32), cat(V, np.float64), cat(B, bool)


def same_bits(got, want, both, msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, msg
    share = float(both.mean()) if both.size else 0.0
    assert share <= 0.05, f"{msg}: the NaN * NaN exemption covers {share:.1%} of the entries"
    g, w = got.view(np.uint64).copy(), want.view(np.uint64).copy()
    if both.any():
        assert np.isnan(got[both]).all(), msg
        g[both] = w[both] = 0
    np.testing.assert_array_equal(g, w, err_msg=msg)


def check(got, want, msg=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    same_bits(got[2], want[2], want[3], msg)


# ---------------------------------------------------------------------------------------------- generators
def make_x(m, ncol, mean_len, rng, empty_every=7):
    lens = np.minimum(rng.integers(max(mean_len // 2, 0), mean_len + mean_len // 2 + 2, size=m), ncol)
    lens[::empty_every] = 0
    p = np.zeros(m + 1, np.int32)
    p[1:] = np.cumsum(lens)
    j = np.concatenate([np.sort(rng.choice(ncol, int(n), replace=False)) for n in lens] + [np.zeros(0, int)])
    x = np.round(rng.normal(size=j.size), 2)
    x[x == 0] = 0.5
    return p, j.astype(np.int32), x


def make_v(kind, L, rng, special=(), frac=0.5):
    """sorted positions, values in the kind's own type, and the positions whose value is not finite / is zero"""
    vi = (np.flatnonzero(rng.random(L) < frac) + 1).astype(np.int32)
    n = vi.size
    if kind == "binary":
        return vi, None
    if kind == "numeric":
        vx = np.round(rng.normal(size=n), 2)
        vx[vx == 0] = 0.25
        for q, s in enumerate(special):
            vx[q * 3 % max(n, 1):q * 3 % max(n, 1) + 1] = s
            if n > 8:
                vx[n - 1 - q] = s
        return vi, vx
    vx = (rng.integers(-3, 4, size=n) if kind == "integer" else rng.integers(0, 2, size=n)).astype(np.int32)
    if special:
        vx[::5] = NA
    return vi, vx


def dirty_x(p, x, L, vi, vxf, rng, share=0.08):
    """NaN / Inf into X: NaNs on rows that v does not store or stores with a finite value; Infs there too, but not
    where the value is 0"""
    m = p.size - 1
    val = np.full(L, np.nan)                                       # nan: not eligible
    stored = np.zeros(L, bool)
    stored[vi - 1] = True
    val[~stored] = 1.0
    val[vi - 1] = 1.0 if vxf is None else np.where(np.isfinite(vxf), vxf, np.nan)
    rows = np.repeat(np.arange(m), np.diff(p))
    v_of = val[rows % L]
    for cand, fill in ((np.flatnonzero(~np.isnan(v_of)), [NA_REAL, OTHER_NAN]),
                       (np.flatnonzero(~np.isnan(v_of) & (v_of != 0)), [np.inf, -np.inf])):
        if cand.size:
            pick = rng.choice(cand, max(int(cand.size * share / 2), min(cand.size, 4)), replace=False)
            x[pick] = np.resize(fill, pick.size)
    return x


def case(m, ncol, mean_len, L, kind, special, dirty, seed, frac=0.5):
    rng = np.random.default_rng(seed)
    p, j, x = make_x(m, ncol, mean_len, rng)
    vi, vx = make_v(kind, L, rng, SPECIALS.get(special, special), frac)
    if dirty:
        x = dirty_x(p, x, L, vi, as_f64(kind, vx), rng)
    return p, j, x, vi, vx


def objects(kind, p, j, x, vi, vx, L, ncol, names=False):
    dn = [[f"r{i}" for i in range(p.size - 1)], [f"c{i}" for i in range(ncol)]] if names else None
    return mx.dgRMatrix(p, j, x, (p.size - 1, ncol), dn), CLS[kind](vi, vx, L)


def run_operator(kind, p, j, x, vi, vx, L, ncol, keep, opts, swap=False, msg=""):
    opts["MatrixExtra.ignore_na"] = not keep
    X, v = objects(kind, p, j, x, vi, vx, L, ncol, names=True)
    out = v * X if swap else X * v
    assert type(out) is mx.dgRMatrix and out.Dim == X.Dim and out.Dimnames == X.Dimnames, msg
    keep_route = keep and kind != "binary"                          # R/operators.R:1606-1614
    check((out.p, out.j, out.x), ref_mul(p, j, x, vi, as_f64(kind, vx), L, ncol, keep_route), msg)
    return out


# ---------------------------------------------------------------------------------------------- sort
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1_000_003])
def test_sort_vector_indices(gpu, n):
    rng = np.random.default_rng(n)
    ii = (rng.permutation(3 * n + 5)[:n] + 1).astype(np.int32)     # unique
    order = np.argsort(ii, kind="stable")
    vals = dict(numeric=rng.normal(size=n), integer=rng.integers(-9, 9, size=n).astype(np.int32),
                logical=rng.integers(0, 2, size=n).astype(np.int32))
    if n:
        vals["numeric"][0], vals["integer"][0] = NA_REAL, NA
    for kind in KINDS:
        i2 = ii.copy()
        if kind == "binary":
            G.sort_vector_indices_binary(i2)
        else:
            x2 = vals[kind].copy()
            getattr(G, "sort_vector_indices_" + kind)(i2, x2)
            want = vals[kind][order]
            np.testing.assert_array_equal(x2.view(np.uint64) if kind == "numeric" else x2,
                                          want.view(np.uint64) if kind == "numeric" else want, err_msg=kind)
        np.testing.assert_array_equal(i2, ii[order], err_msg=kind)
    # already sorted: one reduction, nothing written back
    s_i, s_x = ii[order].copy(), vals["numeric"][order].copy()
    keep_i, keep_x = s_i.copy(), s_x.copy()
    G.sort_vector_indices_numeric(s_i, s_x)
    np.testing.assert_array_equal(s_i, keep_i)
    np.testing.assert_array_equal(s_x.view(np.uint64), keep_x.view(np.uint64))


def test_sorted_vector_takes_the_early_out(gpu):
    """mxd_sort_vector_indices reports whether its one reduction found the vector sorted; the workspace of a sorted
    vector stays as it was (no radix pass ran), and the vector is not written"""
    import ctypes as C
    lib = gpu.load()
    n = 10_000
    for shuffled in (False, True):
        ii = np.arange(1, n + 1, dtype=np.int32) * 3
        if shuffled:
            ii = np.random.default_rng(1).permutation(ii)
        xx = ii.astype(np.float64)
        di, dx = torch.from_numpy(ii).cuda(), torch.from_numpy(xx).cuda()
        nbytes = lib.mxd_sort_vector_indices_workspace_bytes(C.c_int64(n))
        ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        was = C.c_int(-1)
        gpu.check(lib.mxd_sort_vector_indices(C.c_void_p(di.data_ptr()), C.c_void_p(dx.data_ptr()), C.c_int64(n),
                                              C.c_int(gpu.MX_F64), C.c_void_p(ws.data_ptr()), C.byref(was), None))
        torch.cuda.synchronize()
        assert was.value == (0 if shuffled else 1)
        np.testing.assert_array_equal(di.cpu().numpy(), np.sort(ii))
        np.testing.assert_array_equal(dx.cpu().numpy(), np.sort(ii).astype(np.float64))
        untouched = bool((ws[256:] == 0x5A).all())                  # past the flag block: keys, payloads, tables
        assert untouched == (not shuffled)


def test_sort_sparse_indices_of_a_vector(gpu, opts):
    v = mx.dsparseVector([5, 2, 9, 1], [5.0, 2.0, NA_REAL, 1.0], 10)
    s = mx.sort_sparse_indices(v, copy=True)
    assert s is not v and list(v.i) == [5, 2, 9, 1]
    assert list(s.i) == [1, 2, 5, 9] and list(s.x[:3]) == [1.0, 2.0, 5.0] and np.isnan(s.x[3])
    assert mx.sort_sparse_indices(v) is v and list(v.i) == [1, 2, 5, 9]
    n = mx.sort_sparse_indices(mx.nsparseVector([3, 1, 2], None, 3))
    assert list(n.i) == [1, 2, 3]
    mx.check_valid_matrix(s)
    with pytest.raises(mx.MatrixExtraError):
        mx.check_valid_matrix(mx.dsparseVector([1, 11], [1.0, 2.0], 10))


# ---------------------------------------------------------------------------------------------- X * v
@pytest.mark.parametrize("keep", [True, False], ids=["keep_na", "ignore_na"])
@pytest.mark.parametrize("recycles", [1, 2, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_kinds_and_recycling(gpu, opts, kind, recycles, keep):
    m, ncol = 60, 37
    L = m // recycles
    special = "mixed" if kind == "numeric" else ("na" if kind in ("integer", "logical") else "finite")
    args = case(m, ncol, 6, L, kind, special, True, 100 + recycles)
    run_operator(kind, *args, L, ncol, keep, opts, swap=recycles == 2, msg=f"{kind} x{recycles} keep={keep}")


@pytest.mark.parametrize("keep", [True, False], ids=["keep_na", "ignore_na"])
@pytest.mark.parametrize("dirty", [False, True], ids=["clean_X", "dirty_X"])
@pytest.mark.parametrize("special", ["finite", "na", "nan", "pinf", "ninf"])
def test_vector_values(gpu, opts, special, dirty, keep):
    m, ncol, L = 48, 21, 24
    args = case(m, ncol, 5, L, "numeric", special, dirty, 7)
    out = run_operator("numeric", *args, L, ncol, keep, opts, msg=f"{special} dirty={dirty} keep={keep}")
    if keep and special != "finite":
        assert out.j.size > args[1].size // 2                       # some rows were filled


@pytest.mark.parametrize("ncol,mean_len", [(1, 1), (63, 2), (63, 40), (64, 2), (64, 40), (65, 2), (65, 40),
                                           (1000, 2), (1000, 12), (1000, 25), (1000, 40), (1000, 700)])
def test_shapes_and_lane_groups(gpu, opts, ncol, mean_len):
    m, L = 40, 20
    args = case(m, ncol, mean_len, L, "numeric", "mixed", True, ncol + mean_len)
    for keep in (True, False):
        run_operator("numeric", *args, L, ncol, keep, opts, msg=f"ncol={ncol} len={mean_len} keep={keep}")


@pytest.mark.parametrize("keep", [True, False], ids=["keep_na", "ignore_na"])
@pytest.mark.parametrize("dirty", [False, True], ids=["clean_X", "dirty_X"])
def test_vector_storing_nothing(gpu, opts, dirty, keep):
    m, ncol, L = 30, 11, 15
    p, j, x, _, _ = case(m, ncol, 4, L, "numeric", "finite", False, 3)
    vi, vx = np.zeros(0, np.int32), np.zeros(0)
    if dirty:
        x = dirty_x(p, x, L, vi, vx, np.random.default_rng(4))
    out = run_operator("numeric", p, j, x, vi, vx, L, ncol, keep, opts)
    if not (dirty and keep):                                        # operators.cpp:3440-3446, :3516-3522
        assert out.j.size == 0 and out.x.size == 0 and not out.p.any()
    else:
        assert out.j.size == int((~np.isfinite(x)).sum())


@pytest.mark.parametrize("inplace", [False, True], ids=["copies", "inplace_sort"])
def test_unsorted_operands(gpu, opts, inplace):
    m, ncol, L = 40, 30, 20
    p, j, x, vi, vx = case(m, ncol, 8, L, "numeric", "mixed", True, 11)
    rng = np.random.default_rng(12)
    ju, xu = j.copy(), x.copy()
    for r in range(m):
        perm = rng.permutation(p[r + 1] - p[r]) + p[r]
        ju[p[r]:p[r + 1]], xu[p[r]:p[r + 1]] = j[perm], x[perm]
    pv = rng.permutation(vi.size)
    opts["MatrixExtra.inplace_sort"] = inplace
    X, v = mx.dgRMatrix(p, ju.copy(), xu.copy(), (m, ncol)), mx.dsparseVector(vi[pv], vx[pv], L)
    out = X * v
    check((out.p, out.j, out.x), ref_mul(p, j, x, vi, vx, L, ncol, True))
    if inplace:                                                     # a dgRMatrix / dsparseVector is sorted where it is
        np.testing.assert_array_equal(X.j, j)
        np.testing.assert_array_equal(v.i, vi)
    else:
        np.testing.assert_array_equal(X.j, ju)
        np.testing.assert_array_equal(X.x.view(np.uint64), xu.view(np.uint64))
        np.testing.assert_array_equal(v.i, vi[pv])
        np.testing.assert_array_equal(v.x.view(np.uint64), vx[pv].view(np.uint64))


@pytest.mark.parametrize("kind", ["integer", "logical", "binary"])
def test_inplace_sort_of_other_classes(gpu, opts, kind):
    """under inplace_sort an operand that is not of the numeric kind is copied before it is converted and sorted
    (deepcopy_before_sort, R/utils.R:164-191): the caller's lgRMatrix and i/l/nsparseVector stay as they were"""
    m, ncol, L = 24, 13, 12
    p, j, x, vi, vx = case(m, ncol, 5, L, kind, "na" if kind != "binary" else "finite", False, 61)
    rng = np.random.default_rng(62)
    ju = j.copy()
    for r in range(m):
        ju[p[r]:p[r + 1]] = rng.permutation(j[p[r]:p[r + 1]])
    pv = rng.permutation(vi.size)
    opts["MatrixExtra.inplace_sort"] = True
    X = mx.lgRMatrix(p, ju.copy(), np.ones(j.size, np.int32), (m, ncol))
    v = CLS[kind](vi[pv], None if vx is None else vx[pv], L)
    out = X * v
    check((out.p, out.j, out.x), ref_mul(p, j, np.ones(j.size), vi, as_f64(kind, vx), L, ncol, kind != "binary"))
    np.testing.assert_array_equal(X.j, ju)
    np.testing.assert_array_equal(v.i, vi[pv])
    if vx is not None:
        np.testing.assert_array_equal(v.x, vx[pv])


def test_other_matrix_classes_and_dense_routes(gpu, opts):
    m, ncol, L = 20, 9, 10
    p, j, x, vi, vx = case(m, ncol, 4, L, "numeric", "na", False, 21)
    want = ref_mul(p, j, np.ones(j.size), vi, vx, L, ncol, True)
    for X in (mx.ngRMatrix(p, j, None, (m, ncol)), mx.lgRMatrix(p, j, np.ones(j.size, np.int32), (m, ncol))):
        out = X * mx.dsparseVector(vi, vx, L)
        assert type(out) is mx.dgRMatrix
        check((out.p, out.j, out.x), want)
    # every position stored: the dense-vector route with the sorted values (R/operators.R:1570-1581)
    X = mx.dgRMatrix(p, j, x, (m, ncol))
    full = np.round(np.random.default_rng(5).normal(size=L), 2) + 3.0
    perm = np.random.default_rng(6).permutation(L)
    out = X * mx.dsparseVector((perm + 1).astype(np.int32), full[perm], L)
    want = X * full
    np.testing.assert_array_equal(out.x, want.x)
    assert out.p is X.p and out.j is X.j
    out1 = X * mx.dsparseVector([1], [2.0], 1)                       # length 1: as.numeric(v)
    np.testing.assert_array_equal(out1.x, x * 2.0)


def test_both_factors_nan(gpu, opts):
    """the one case where a NaN of v meets a NaN of X: under ignore_na the product keeps some NaN"""
    m, ncol, L = 8, 30, 8
    p, j, x, _, _ = case(m, ncol, 28, L, "numeric", "finite", False, 31, )
    vi, vx = np.arange(1, 9, dtype=np.int32), np.full(8, 1.5)
    vi = vi[[0, 1, 2, 3, 4, 5, 7]]                                  # position 7 not stored: not the dense route
    vx = vx[:7].copy()
    vx[1] = OTHER_NAN
    x[p[1]] = NA_REAL                                               # row 1 is not empty (rows 0 and 7 are)
    assert p[2] > p[1]
    want = ref_mul(p, j, x, vi, vx, L, ncol, False)
    assert want[3].sum() == 1
    run_operator("numeric", p, j, x, vi, vx, L, ncol, False, opts)


def test_exports_and_device_route(gpu):
    m, ncol, L = 50, 33, 25
    p, j, x, vi, vx = case(m, ncol, 10, L, "numeric", "mixed", True, 41)
    for keep in (True, False):
        want = ref_mul(p, j, x, vi, vx, L, ncol, keep)
        got = (G.multiply_csr_by_svec_keep_NAs(p, j, x, vi, vx, ncol, L) if keep
               else G.multiply_csr_by_svec_no_NAs(p, j, x, vi, vx, L))
        check((got["indptr"], got["indices"], got["values"]), want, f"export keep={keep}")
        A = Dv.DeviceCSR.from_host(p, j, x, ncol)
        dp, dj, dx = Dv.csr_by_svec(A, torch.from_numpy(vi).cuda(), torch.from_numpy(vx).cuda(), L, keep_na=keep)
        torch.cuda.synchronize()
        check((dp.cpu().numpy(), dj.cpu().numpy(), dx.cpu().numpy()), want, f"device keep={keep}")
    # an nsparseVector through the keep-NAs export: rows copied, NaN / Inf of dropped rows kept (:3573, :3603-3607)
    got = G.multiply_csr_by_svec_keep_NAs(p, j, x, vi, np.zeros(0), ncol, L)
    check((got["indptr"], got["indices"], got["values"]), ref_mul(p, j, x, vi, None, L, ncol, True), "binary keep")
    with pytest.raises(mx._lib.MxError, match="must divide"):
        G.multiply_csr_by_svec_no_NAs(p, j, x, vi, vx, 7)


def test_large_case(gpu, opts):
    """200 000 x 300, length(v) = 1000 storing 30 %, 1 % of the stored values NaN / Inf: many blocks, and dense-filled
    rows spread over the whole output"""
    m, ncol, L = 200_000, 300, 1000
    rng = np.random.default_rng(2024)
    lens = rng.integers(0, 17, size=m)
    p = np.zeros(m + 1, np.int32)
    p[1:] = np.cumsum(lens)
    gaps = rng.integers(1, ncol // 16, size=int(p[-1]))
    run = np.cumsum(gaps)
    first = p[:-1][lens > 0]
    j = (run - np.repeat(run[first] - gaps[first], lens[lens > 0])).astype(np.int32)     # ascending inside a row
    assert j.min() >= 1 and j.max() < ncol
    x = np.round(rng.normal(size=j.size), 2)
    x[x == 0] = 0.5
    vi = (np.sort(rng.choice(L, 300, replace=False)) + 1).astype(np.int32)
    vx = np.round(rng.normal(size=300), 2)
    vx[vx == 0] = 0.25
    vx[[10, 150, 290]] = [NA_REAL, np.inf, -np.inf]
    x = dirty_x(p, x, L, vi, vx, rng, share=0.001)
    out = run_operator("numeric", p, j, x, vi, vx, L, ncol, True, opts, msg="large")
    assert out.j.size > 3 * (m // L) * ncol


# ---------------------------------------------------------------------------------------------- X %*% v
@pytest.mark.parametrize("kind", KINDS)
def test_matmul_sparse_vector(gpu, opts, kind):
    m, ncol = 70, 45
    rng = np.random.default_rng(51)
    p, j, x = make_x(m, ncol, 9, rng)
    vi, vx = make_v(kind, ncol, rng)
    pv = rng.permutation(vi.size)
    X, _ = objects(kind, p, j, x, vi, vx, ncol, ncol, names=True)
    v = CLS[kind](vi[pv], None if vx is None else vx[pv], ncol)
    got = X @ v
    dense = np.zeros(ncol)
    dense[vi - 1] = 1.0 if vx is None else vx.astype(np.float64)
    want = X @ dense
    assert isinstance(got, mx.DenseMatrix) and got.shape == (m, 1)
    assert got.Dimnames[0] == X.Dimnames[0] and got.Dimnames[1] is None
    np.testing.assert_allclose(np.asarray(got), np.asarray(want), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(v.i, vi[pv])                      # sorted on a copy
    with pytest.raises(mx.MatrixExtraError, match="Matrix-vector dimensions do not match."):
        X @ CLS[kind](vi, vx, ncol + 1)
    # under inplace_sort the vector and a dgRMatrix are sorted where they are (R/matmul.R:598-603)
    ju = j.copy()
    for r in range(m):
        ju[p[r]:p[r + 1]] = ju[p[r]:p[r + 1]][::-1]
    xu = np.concatenate([x[p[r]:p[r + 1]][::-1] for r in range(m)])
    opts["MatrixExtra.inplace_sort"] = True
    Xu = mx.dgRMatrix(p, ju, xu, (m, ncol))
    got2 = Xu @ v
    np.testing.assert_allclose(np.asarray(got2), np.asarray(want), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(v.i, vi)
    np.testing.assert_array_equal(Xu.j, j)
