"""The CPU restatement (oracle/mx_oracle.c through oracle/oracle.py) against the reference's own compiled C++.

Two layers: the committed reference-run fixture (tests/golden/reference_golden.npz, always), and the live library
oracle/_ref/libmxref.so on a wider seeded sweep (whenever it is built or can be built).  Bars: tests/refpin.py."""
import os

import numpy as np
import pytest

import refpin
from conftest import rand_csr
from oracle import oracle as O
from oracle import ref as Ref

RECORDS, META = refpin.load()
IN_ORACLE = [r for r in RECORDS if refpin.has(O, r.fn)]


def _live():
    if not Ref.available() and Ref.sources_present():
        Ref.build()
    return Ref.available()


needs_ref = pytest.mark.skipif(not _live(), reason="neither oracle/_ref/libmxref.so nor the reference's sources are here")


def test_fixture_says_what_made_it():
    assert "-ffp-contract=off" in META["compile_flags"] and "-O2" in META["compile_flags"]
    assert int(META["seed"]) > 0
    assert os.path.getsize(refpin.PATH) < 300 * 1024
    assert len({r.fn for r in RECORDS}) >= 85


def test_every_oracle_routine_is_pinned():
    """Each routine that oracle.py restates has at least one reference-run record."""
    names = [n for n in dir(O) if not n.startswith("_") and callable(getattr(O, n)) and getattr(O, n).__doc__
             and "src/" in getattr(O, n).__doc__]
    pinned = {r.fn for r in RECORDS}
    renamed = {"sort_sparse_indices": "sort_sparse_indices_numeric",
               "reverse_columns_inplace": "reverse_columns_inplace_numeric", "gemm_csr_drm_as_drm": "matmul_dense_csc_numeric",
               "gemm_csr_drm_as_dcm": "tcrossprod_csr_dense_numeric", "tcrossprod_csr_dense": "tcrossprod_csr_dense_numeric",
               "matmul_dense_csc": "matmul_dense_csc_numeric", "tcrossprod_dense_csr": "tcrossprod_dense_csr_numeric"}
    missing = [n for n in names if renamed.get(n, n) not in pinned]
    assert not missing, missing


@pytest.mark.parametrize("rec", IN_ORACLE, ids=[f"{n:03d}-{r!r}" for n, r in enumerate(IN_ORACLE)])
def test_oracle_reproduces_the_reference_run(rec):
    got, live = refpin.replay(O, rec)
    if rec.err is not None:                   # oracle.py raises ValueError with the reference's message
        assert isinstance(got, Exception) and rec.err in str(got)
        return
    refpin.compare(rec, got, live, device=False)


@needs_ref
@pytest.mark.parametrize("rec", RECORDS, ids=[f"{n:03d}-{r!r}" for n, r in enumerate(RECORDS)])
def test_fixture_is_what_the_reference_returns_now(rec):
    """The committed file is a run of this reference with these flags: every record is made again, bit for bit."""
    got, live = refpin.replay(Ref, rec)
    refpin.compare(rec, got, live, device=False)


@needs_ref
def test_no_reference_object_outlives_its_call():
    Ref.call("check_is_seq", np.arange(3, dtype=np.int32))
    assert Ref.live_objects() == 0


@needs_ref
def test_aliasing_survives_the_stand_in():
    p, j, x = rand_csr(9, 7, 0.5, seed=3)
    r = Ref.multiply_csr_elemwise(p, p, j, j, x, x)
    assert r["indptr"] is p and r["indices"] is j and r["values"] is not x
    r = Ref.multiply_csr_elemwise(p, p.copy(), j, j.copy(), x, x)
    assert r["indptr"] is not p and np.array_equal(r["indptr"], p)
    assert Ref.is_same_ngRMatrix(p, p, j, j) and not Ref.is_same_ngRMatrix(p, p.copy(), j, j)


# ----------------------------------------------------------------------------- live, wider sweep
SWEEP = [(m, K, d, s) for s, (m, K, d) in enumerate([(1, 1, 1.0), (7, 5, 0.5), (33, 17, 0.2), (64, 40, 0.1), (120, 9, 0.6),
                                                      (200, 64, 0.05)])]


def _both(fn, *args):
    rec = refpin.capture(Ref, fn, args)
    got, live = refpin.replay(O, rec)
    refpin.compare(rec, got, live, device=False)


@needs_ref
@pytest.mark.parametrize("m,K,dens,seed", SWEEP)
def test_live_products(m, K, dens, seed):
    p, j, x = rand_csr(m, K, dens, seed=900 + seed, sorted_cols=False)
    rng = np.random.default_rng(910 + seed)
    for n in sorted({1, min(m, 5), m}):
        Y = np.asfortranarray(rng.normal(size=(n, K)))
        _both("tcrossprod_csr_dense_numeric", p, j, x, Y, 1)
        _both("tcrossprod_csr_dense_float32", p, j, x, Y.astype(np.float32), 1)
    X = np.asfortranarray(rng.normal(size=(m + 4, K)))
    _both("matmul_dense_csc_numeric", X, p, j, x, 1)
    _both("matmul_dense_csc_float32", X.astype(np.float32), p, j, x, 1)
    _both("tcrossprod_dense_csr_numeric", X, p, j, x, 1, K)
    _both("tcrossprod_dense_csr_float32", X.astype(np.float32), p, j, x, 1, K)
    _both("matmul_csr_dvec_numeric", p, j, x, rng.normal(size=K), 1)
    yi = rng.integers(-5, 5, size=K).astype(np.int32); yi[::4] = -2147483648
    _both("matmul_csr_dvec_integer", p, j, x, yi, 1)
    _both("matmul_csr_dvec_logical", p, j, x, (yi > 0).astype(np.int32), 1)
    _both("matmul_csr_dvec_float32", p, j, x, rng.normal(size=K).astype(np.float32), 1)


@needs_ref
@pytest.mark.parametrize("m,K,dens,seed", SWEEP)
def test_live_merges_gathers_binds(m, K, dens, seed):
    a = rand_csr(m, K, dens, seed=920 + seed)
    b = rand_csr(m, K, min(1.0, dens * 1.5), seed=930 + seed)
    for sub in (False, True):
        _both("add_csr_elemwise", a[0], b[0], a[1], b[1], a[2], b[2], sub)
        _both("add_csr_elemwise", a[0], a[0], a[1], a[1], a[2], a[2], sub)
    _both("multiply_csr_elemwise", a[0], b[0], a[1], b[1], a[2], b[2])
    la, lb = rand_csr(m, K, dens, seed=940 + seed, dtype="l"), rand_csr(m, K, dens, seed=950 + seed, dtype="l")
    for xor in (False, True):
        _both("logicalor_csr_elemwise", la[0], lb[0], la[1], lb[1], la[2], lb[2], xor)
    _both("logicaland_csr_elemwise", la[0], lb[0], la[1], lb[1], la[2], lb[2])
    rng = np.random.default_rng(960 + seed)
    rows = rng.integers(0, m, size=m + 3).astype(np.int32)
    cols = rng.integers(0, K, size=K + 2).astype(np.int32)
    _both("copy_csr_rows_numeric", a[0], a[1], a[2], rows)
    _both("copy_csr_rows_logical", la[0], la[1], la[2], rows)
    _both("copy_csr_rows_binary", a[0], a[1], rows)
    lo, hi = sorted(rng.integers(0, K, size=2).tolist())
    _both("copy_csr_rows_col_seq_numeric", a[0], a[1], a[2], rows, np.arange(lo, hi + 1, dtype=np.int32), False)
    _both("copy_csr_rows_col_seq_logical", la[0], la[1], la[2], rows, np.arange(lo + 1, hi + 2, dtype=np.int32), True)
    _both("copy_csr_rows_col_seq_binary", a[0], a[1], rows, np.arange(lo, hi + 1, dtype=np.int32), False)
    _both("copy_csr_arbitrary_numeric", a[0], a[1], a[2], rows, cols)
    _both("copy_csr_arbitrary_logical", la[0], la[1], la[2], rows, cols)
    _both("reverse_rows_numeric", a[0], a[1], a[2])
    _both("reverse_rows_logical", la[0], la[1], la[2])
    _both("reverse_rows_binary", a[0], a[1])
    _both("reverse_columns_inplace_numeric", a[0], a[1], a[2], K)
    _both("cbind_csr_numeric", a[0], a[1], a[2], b[0], b[1] + K, b[2])
    _both("cbind_csr_logical", la[0], la[1], la[2], lb[0], lb[1] + K, lb[2])
    _both("cbind_csr_binary", a[0], a[1], b[0], b[1] + K)
    _both("concat_indptr2", a[0], b[0])
    vi = np.sort(rng.choice(np.arange(1, K + 1), size=max(1, K // 3), replace=False)).astype(np.int32)
    objs = [(0, a[0], a[1], a[2]), (1, la[0], la[1], la[2]), (2, b[0], b[1], None), (3, None, vi, rng.normal(size=vi.size)),
            (4, None, vi, rng.integers(-3, 4, size=vi.size).astype(np.int32)), (5, None, vi, la[2][:vi.size] if la[2].size >= vi.size
                                                                                else np.ones(vi.size, np.int32)), (6, None, vi, None)]
    for out_kind in (0, 1, 2):
        _both("concat_csr_batch", np.array([o[0] for o in objs], np.int32), np.array([m, m, m, 1, 1, 1, 1], np.int32), out_kind,
              *[o[k] for o in objs for k in (1, 2, 3)])
    u = rand_csr(m, K, dens, seed=970 + seed, sorted_cols=False)
    _both("sort_sparse_indices_numeric", u[0], u[1], u[2])
    _both("check_indices_are_sorted", u[0], u[1])
    _both("check_indices_are_sorted", a[0], a[1])


@needs_ref
@pytest.mark.parametrize("m,K,dens,seed", SWEEP)
def test_live_vector_operators(m, K, dens, seed):
    p, j, x = rand_csr(m, K, dens, seed=980 + seed)
    rng = np.random.default_rng(990 + seed)
    x = x.copy(); x[::11] = np.inf; x[5::13] = np.nan; x[7::17] = -0.0
    for L in sorted({1, m, m * K, max(1, m // 2), m + 1}):
        v = rng.uniform(0.01, 50.0, size=L) * rng.choice([-1.0, 1.0], size=L)
        if L > 3:
            v[1], v[2] = np.exp2(rng.uniform(-40, 40)), -np.exp2(rng.uniform(-40, 40))
        for o in range(5):
            for lhs in (True, False):
                _both("multiply_csr_by_dvec_no_NAs_numeric", p, j, x, v, K, *[k == o for k in range(5)], lhs)
        _both("logicaland_csr_by_dvec_internal", p, j, (x > 0).astype(np.int32), (v > 0).astype(np.int32), K)
    D = rng.normal(size=(m, K))
    _both("multiply_csr_by_dense_elemwise_double", p, j, x, np.asfortranarray(D))
    _both("multiply_csr_by_dense_elemwise_float32", p, j, x, np.asfortranarray(D.astype(np.float32)))
    Di = rng.integers(-3, 4, size=(m, K)).astype(np.int32); Di[rng.random((m, K)) < 0.2] = -2147483648
    _both("multiply_csr_by_dense_elemwise_int", p, j, x, np.asfortranarray(Di))
    _both("multiply_csr_by_dense_elemwise_bool", p, j, x, np.asfortranarray(Di))
    _both("logicaland_csr_by_dense_cpp", p, j, Di.reshape(-1)[:j.size].copy(), np.asfortranarray(Di))
    ii = np.sort(rng.choice(np.arange(1, K + 1), size=max(1, K // 2), replace=False)).astype(np.int32)
    _both("matmul_csr_svec_numeric", p, j, x, ii, rng.normal(size=ii.size), 1)
    _both("matmul_csr_svec_binary", p, j, x, ii, 1)
    yv = rng.integers(-3, 4, size=ii.size).astype(np.int32); yv[::3] = -2147483648
    _both("matmul_csr_svec_integer", p, j, x, ii, yv, 1)
    _both("matmul_csr_svec_logical", p, j, x, ii, yv, 1)
    _both("matmul_csr_svec_float32", p, j, x, ii, rng.normal(size=ii.size).astype(np.float32), 1)
