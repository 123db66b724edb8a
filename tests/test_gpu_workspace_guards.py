"""Every caller-allocated workspace of the two-pass device entries, exactly mxd_*_workspace_bytes long and between
guard bytes (tests/devmem.py), with the inputs and outputs guarded too.  A layout (csrc/mx_workspace.h) whose segment
lies past the published size writes into the back guard; one whose segments overlap gives a wrong result, which is
compared with the expectation of the family's own test (their oracles and models are imported; the mask rule of the
compaction and the single-cell lookup, whose tests state the expectation inline, use the same expressions).

Sizes: the driving size at 1 and at one tile + 1 (4096 entries or cells a tile in compact.hip, cscdense.hip and
transpose.hip), so that a segment behind a per-tile array starts at an offset of its own; where a segment follows a
count block sized by an entry count, also 2^18 + 1 entries, the first size at which the scan workspace inside that
block holds several tile sums.  The transpose family also takes an nnz with nnz % 4 == 2, and both its sizes have
nnz % 4 and (nnz + 1) % 4 non-zero, so that the padded sizes of its nnz and nnz + 1 arrays differ."""
import numpy as np
import pytest

import coo_sort_model as CM
import dense_svec_model as DM
import devmem
import dvec_na_model as NM
import matrixextra_amd as mx
import test_gpu_coo as TC
import test_gpu_coo_slice as TS
import test_gpu_csc_dense as TD
import test_gpu_outer as TO
import test_gpu_sparse_cleanup as TL
import test_gpu_transpose as TT
from conftest import rand_csr
from matrixextra_amd import _lib
from test_gpu_coo_sort import check_against_model as check_coo_sort

pytestmark = pytest.mark.gpu

TILE1 = 4096 + 1
SCAN1 = 2**18 + 1                      # one past what scan.hip scans in a single workgroup
NA = np.int32(-2147483648)
NA_REAL = mx.NA_REAL


# ----------------------------------------------------------------------------- CSC (.) dense, NA cells kept
@pytest.mark.parametrize("kind", ["numeric", "integer"])
@pytest.mark.parametrize("m,n", [(1, 1), (17, 241)])                # 1 and 4097 cells
def test_csc_dense_na(gpu, m, n, kind):
    p, i, x = TD.csc_case(m, n, 0.3, seed=m + n)
    D = TD.dense_of(kind, m, n, np.random.default_rng(3 * m + n))
    D[0, 0] = D[m - 1, n - 1] = NA_REAL if kind == "numeric" else NA
    ep, ei, ev, both = TD.ref_keep(kind, p, i, x, D)
    assert ei.size > i.size or m == 1
    got = devmem.dev_csc_dense_na(p, i, x, D, TD.KINDS.index(kind))
    np.testing.assert_array_equal(got[0], ep)
    np.testing.assert_array_equal(got[1], ei)
    TD.same_bits(got[2], ev, both)


# ----------------------------------------------------------------------------- CSR (op) dense vector, NA cells kept
@pytest.mark.parametrize("m,L", [(1, 1), (TILE1, 17)])
def test_dvec_na_rows(gpu, m, L):
    op, ncols = "/", 5
    p, j, x = NM.make_csr(m, ncols, 0.3, seed=m)
    v = NM.make_vector(L, op, seed=L, at=(0, L - 1))
    exp = NM.model(p, j, x, v, ncols, op)
    NM.compare(devmem.dev_dvec_na_rows(p, j, x, ncols, v, op), exp, op)


def _all_special(L):
    return np.array([NA_REAL, NM.OTHER_NAN, np.inf] * L)[:L]


DVEC_FLAT = {   # m, ncols, the vector, its candidate cells (None: whatever the model finds)
    # a length of 1 divides every row count and takes the row-ruled route: 2 is the flat route's smallest
    "length_2": (3, 3, np.array([NA_REAL, 2.0]), 5),
    "one_candidate": (3, 3, np.where(np.arange(9) == 4, NA_REAL, 1.5), 1),
    "candidates_tile+1": (17, 241, _all_special(3), TILE1),
    "length_tile+1": (300, 130, NM.make_vector(TILE1, "*", seed=9, at=(0, TILE1 - 1), share=0.02), None),
    "candidates_2^18+1": (5, 52429, _all_special(3), SCAN1),
}


@pytest.mark.parametrize("case", list(DVEC_FLAT))
def test_dvec_na_special_cells_and_join(gpu, case):
    m, ncols, v, candidates = DVEC_FLAT[case]
    op = "*"
    p, j, x = NM.make_csr(m, ncols, 0.1 if m * ncols < 10**5 else 0.01, seed=m, empty_rows=(1,))
    exp = NM.model(p, j, x, v, ncols, op)
    got, nsp, cand, new = devmem.dev_dvec_na_flat(p, j, x, ncols, v, op)
    assert nsp == int(NM.special(op, v).sum()) and cand == exp["candidates"] and new == exp["new"]
    assert candidates is None or cand == candidates
    NM.compare(got, exp, op)


# ----------------------------------------------------------------------------- dense * sparse vector
@pytest.mark.parametrize("nrows,ncols,length,kind", [(1, 1, 1, "numeric"), (5, 3, 15, "numeric"), (2, 3, 1, "numeric"),
                                                     (TILE1, 2, TILE1, "numeric"), (TILE1, 2, 17, "integer")])
def test_dense_by_svec(gpu, nrows, ncols, length, kind):
    X, ii, xx = DM.svec_case(kind, nrows, ncols, length, "some", seed=nrows + length)
    want, both = DM.model(kind, X, ii, xx, length, True)
    got = devmem.dev_dense_by_svec(X, DM.KINDS.index(kind), ii, xx, length, True)
    DM.compare_results(got, want, both, f"{kind} {nrows} x {ncols}, length {length}")


# ----------------------------------------------------------------------------- outer products
@pytest.mark.parametrize("m", [1, TILE1])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_outer_dense(gpu, m, f32):
    p, _, x = TO.one_column(m, "none_empty" if m == 1 else "mixed", seed=m)
    v = TO.dense_vector(3, seed=7)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = v.astype(np.float32) if f32 else v
    want = TO.model_dense(v, p, x, f32)
    TO.same_triple(devmem.dev_outer_dense(p, x, v), want, f"m={m}")


@pytest.mark.parametrize("m,length", [(1, 1), (TILE1, 5), (3, TILE1)])
def test_outer_svec(gpu, m, length):
    p, _, x = TO.one_column(m, "none_empty" if m < 4 else "mixed", seed=m)
    yi = np.unique(np.array([1, (length + 1) // 2, length], dtype=np.int32))
    yv = TO.svec_values("numeric", yi.size, seed=length)
    want = TO.model_svec(p, x, yi, yv, length, "numeric")
    TO.same_triple(devmem.dev_outer_svec(p, x, yi, yv, _lib.MX_F64, length), want, f"m={m} length={length}")


# ----------------------------------------------------------------------------- COO slices
@pytest.mark.parametrize("nnz,kind", [(1, "d"), (TILE1, "d"), (TILE1, "l"), (TILE1, "n"), (SCAN1, "d")])
def test_coo_slice(gpu, nnz, kind):
    m, n, lo, hi = 37, 23, 3, 19
    T = TS.make_coo(m, n, nnz, kind, seed=nnz, dup_share=0.0)
    rng = np.random.default_rng(nnz + 1)
    take = rng.integers(1, m + 1, size=20).astype(np.int32)         # repeats, any order
    take[0], T.j[0] = T.i[0] + 1, lo + 2                            # the one entry of the smallest case is selected
    j1 = np.arange(lo + 1, hi + 2)
    want = TS.ref_slice(T.i, T.j, T.x, take, j1, m, n)
    got = devmem.dev_coo_slice(T.i, T.j, T.x, m, n, take, lo, hi)
    assert want[0].size > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    TS.assert_bits(got[2], want[2])


@pytest.mark.parametrize("nnz", [1, TILE1])
def test_coo_single(gpu, nnz):
    T = TS.make_coo(37, 23, nnz, "d", seed=nnz)
    for r, c in [(int(T.i[-1]), int(T.j[-1])), (int(T.i[0]), int(T.j[0])), (37, 23)]:
        hits = np.flatnonzero((T.i == r) & (T.j == c))
        k, value = devmem.dev_coo_single(T.i, T.j, T.x, r, c)
        assert k == (int(hits[0]) if hits.size else -1)
        assert not hits.size or value == T.x[hits[0]].tobytes()


# ----------------------------------------------------------------------------- CSR (.) COO
@pytest.mark.parametrize("nnz_y", [1, TILE1, SCAN1])
def test_csr_by_coo(gpu, nnz_y):
    p, j, x = rand_csr(30, 20, 0.3, 9)
    X = mx.dgRMatrix(p, j, x, (30, 20))
    yi, yj, y = TC.rand_coo(35, 25, nnz_y, nnz_y, dup_share=0.1 if nnz_y > 1 else 0.0)
    if nnz_y == SCAN1:                                              # the restatement is a Python loop over non-zeros
        y[np.random.default_rng(1).random(nnz_y) < 0.98] = 0.0
    yi[-1], yj[-1], y[-1] = np.flatnonzero(np.diff(p))[0], j[0], 2.0   # the last entry of y meets a stored cell
    r, c, v = TC.ref_csr_by_coo(X, yi, yj, y, False)
    assert r.size > 0
    got = devmem.dev_csr_by_coo(False, p, j, x, 20, yi, yj, y)
    assert np.array_equal(got[0], r) and np.array_equal(got[1], c)
    TC.assert_bits(got[2], v)


# ----------------------------------------------------------------------------- compaction
def _rows_over(n, m, rng):
    p = np.zeros(m + 1, dtype=np.int32)
    p[1:-1] = np.sort(rng.integers(0, n + 1, size=m - 1))
    p[-1] = n
    return p


@pytest.mark.parametrize("n", [1, TILE1])
@pytest.mark.parametrize("entry", ["zero_rule", "mask"])
def test_compact(gpu, n, entry):
    rng = np.random.default_rng(n)
    p, j = _rows_over(n, 50, rng), rng.integers(0, 500, size=n).astype(np.int32)
    x = TL.values_of("d", n, rng)
    if entry == "zero_rule":                                        # remove_sparse_zeros
        x[0] = 1.5
        keep, want = TL.ref_keep("csr", "d", x, False), x
        got = devmem.dev_compact(p, j, x, _lib.MX_KEEP_NONZERO)
    else:                                                           # filterSparse: an NA in the mask keeps the entry, as NA
        mask = rng.choice(np.array([0, 1, NA], np.int32), size=n)
        mask[0] = NA
        keep, want = mask != 0, np.where(mask == NA, NA_REAL, x)
        got = devmem.dev_compact(p, j, x, _lib.MX_KEEP_MASK, mask)
    assert got[3] == keep.sum() > 0
    np.testing.assert_array_equal(got[0], TL.ref_indptr(p, keep))
    np.testing.assert_array_equal(got[1], j[keep])
    TL.same_values(got[2], want[keep])


# ----------------------------------------------------------------------------- the transpose family
NNZS = [1, TILE1, 10002]
assert all(k % 4 and (k + 1) % 4 for k in NNZS) and 10002 % 4 == 2


def _values(kind, n, rng):
    return {"d": lambda: np.round(rng.normal(size=n), 3),
            "l": lambda: rng.choice(np.array([0, 1, NA], dtype=np.int32), size=n), "n": lambda: None}[kind]()


def _csr_with(nnz, m, ncol, kind, dup, seed):
    """exactly nnz entries, columns in any order inside a row; dup: drawn with replacement from few cells"""
    rng = np.random.default_rng(seed)
    if dup:
        rows, j = np.sort(rng.integers(0, m, size=nnz)), rng.integers(0, ncol, size=nnz).astype(np.int32)
    else:
        flat = rng.choice(m * ncol, size=nnz, replace=False)
        flat = flat[np.argsort(flat // ncol, kind="stable")]        # by row, the columns of a row as they were drawn
        rows, j = flat // ncol, (flat % ncol).astype(np.int32)
    p = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return p, j, _values(kind, nnz, rng)


TRANSPOSE = [(1, "d", False), (TILE1, "d", False), (TILE1, "l", False), (TILE1, "n", False), (10002, "d", False),
             (TILE1, "d", True), (TILE1, "l", True), (10002, "n", True)]


@pytest.mark.parametrize("nnz,kind,dup", TRANSPOSE)
def test_csr_transpose(gpu, nnz, kind, dup):
    m, ncol = (40, 8) if dup else (200, 300)                        # 320 cells: the compaction merges most entries
    p, j, x = _csr_with(nnz, m, ncol, kind, dup, seed=nnz)
    ip, ij, iv = TT.ref_transpose(p, j, x, ncol)
    assert (ij.size < nnz) == dup
    got = devmem.dev_csr_transpose(p, j, x, ncol)
    assert np.array_equal(got[0], ip) and np.array_equal(got[1], ij)
    TT.assert_bits(got[2], iv)


@pytest.mark.parametrize("nnz,kind,dup", TRANSPOSE + [(TILE1, "d", "wide")])
def test_coo_to_csr(gpu, nnz, kind, dup):
    m, n = (40, 8) if dup is True else (300, TILE1) if dup == "wide" else (300, 200)    # wide: a CSC of 4098 pointers
    i, j, _ = TC.rand_coo(m, n, nnz, seed=nnz, kind="n")
    x = _values(kind, nnz, np.random.default_rng(nnz))
    ip, ij, iv = TC.ref_coo_to_csr(i, j, x, m, n)
    assert dup is not True or ij.size < nnz
    got = devmem.dev_coo_to_csr(i, j, x, m, n)
    assert np.array_equal(got[0], ip) and np.array_equal(got[1], ij)
    TC.assert_bits(got[2], iv)


@pytest.mark.parametrize("nnz,kind,dup", [(n, {"d": "numeric", "l": "logical", "n": "binary"}[k], d)
                                          for n, k, d in TRANSPOSE])
def test_coo_sort(gpu, nnz, kind, dup):
    rng = np.random.default_rng(nnz)
    i, j = CM.repeated_cells(40, 8, nnz, rng) if dup else CM.unique_cells(300, 300, nnz, rng)
    check_coo_sort(i, j, CM.values_for(kind, nnz, rng), kind, f"nnz {nnz} {kind}", expect_sorted=nnz < 2)


@pytest.mark.parametrize("n", [1, 2] + NNZS[1:])
@pytest.mark.parametrize("vd", ["MX_F64", "MX_I32", "MX_NONE"])
def test_sort_vector_indices(gpu, n, vd):
    rng = np.random.default_rng(n)
    ii = (rng.permutation(3 * n + 5)[:n] + 1).astype(np.int32)      # unique
    if n == 2:
        ii = np.array([9, 4], dtype=np.int32)
    xx = {"MX_F64": rng.normal(size=n), "MX_I32": rng.integers(-9, 9, size=n).astype(np.int32), "MX_NONE": None}[vd]
    order = np.argsort(ii, kind="stable")
    gi, gx, was = devmem.dev_sort_vector(ii, xx, getattr(_lib, vd))
    assert was == int(n < 2)
    np.testing.assert_array_equal(gi, ii[order])
    if xx is not None:
        np.testing.assert_array_equal(gx.view(np.uint8), xx[order].view(np.uint8))
