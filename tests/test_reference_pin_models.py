"""The numpy restatements that the larger-shape GPU tests use as their yardstick, held to the reference's own
compiled C++: tests/dvec_na_model.model and the ref_* functions of the GPU test modules.  Against the committed
reference-run fixture always, and against oracle/_ref/libmxref.so live on other seeds where it is built.  Each model
is compared the way its own GPU test compares the device with it.  No GPU is used."""
from types import SimpleNamespace

import numpy as np
import pytest

import dvec_na_model as DM
import refpin
import test_gpu_coo as TCOO
import test_gpu_coo_slice as TSLICE
import test_gpu_csc_dense as TCSC
import test_gpu_sparse_cleanup as TCLEAN
import test_gpu_svec_operands as TSVEC
from conftest import rand_csr
from oracle import ref as Ref

RECORDS, _META = refpin.load()
NA = np.int32(-2147483648)


def _bits(a, b, what):
    refpin.exact(np.asarray(a), np.asarray(b), what, nan_bits=np.ones(np.asarray(b).size, dtype=bool))


# ----------------------------------------------------------------------------- one check per model
def check_dvec_na(rec):
    p, j, x, v, ncols = rec.args[:5]
    op = DM.OPS[[bool(f) for f in rec.args[5:10]].index(True)]
    exp = DM.model(p, j, x, v, ncols, op, bool(rec.args[10]))
    DM.compare(rec.out, exp, op)
    assert bool(exp["alias"]) == ("indptr" in rec.alias), f"{rec!r}: alias flag"


def check_svec(rec):
    keep = rec.fn.endswith("keep_NAs")
    p, j, x, vi, xx = rec.args[:5]
    ncol, L = (rec.args[5], rec.args[6]) if keep else (0, rec.args[5])
    vx = None if (xx.size == 0 and vi.size) else xx
    TSVEC.check((rec.out["indptr"], rec.out["indices"], rec.out["values"]), TSVEC.ref_mul(p, j, x, vi, vx, L, ncol, keep), repr(rec))


def check_csc(rec):
    kind = "and" if rec.fn.startswith("logicaland") else rec.fn.rsplit("_", 1)[1]
    p, i, x, D = rec.args
    if "ignore" in rec.fn:
        want, both = TCSC.ref_ignore(kind, p, i, x, D)
        TCSC.same_bits(rec.out, want, both, repr(rec))
    else:
        ep, ei, ev, both = TCSC.ref_keep(kind, p, i, x, D)
        np.testing.assert_array_equal(rec.out["indptr"], ep)
        np.testing.assert_array_equal(rec.out["indices"], ei)
        TCSC.same_bits(rec.out["values"], ev, both, repr(rec))


def check_cleanup(rec):
    _, _, _, layout, kind = rec.fn.split("_")
    kind = {"numeric": "d", "logical": "l", "integer": "i"}[kind]
    x, na_rm = rec.args[-2], rec.args[-1]
    keep = TCLEAN.ref_keep(layout, kind, x, na_rm)
    out = rec.out
    if layout == "csr":
        np.testing.assert_array_equal(out["indptr"], TCLEAN.ref_indptr(rec.args[0], keep))
        np.testing.assert_array_equal(out["indices"], rec.args[1][keep])
        _bits(out["values"], x[keep], repr(rec))           # the fixture holds the defined half for the logical kind
    elif layout == "coo":
        np.testing.assert_array_equal(out["ii"], rec.args[0][keep])
        np.testing.assert_array_equal(out["jj"], rec.args[1][keep])
        _bits(out["xx"], x[keep], repr(rec))
    else:
        np.testing.assert_array_equal(out["ii"], rec.args[0][keep])
        kept = x[keep]
        if kind == "d" and "xx" not in rec.alias:          # the reference truncates here: model keeps doubles
            fin = np.isfinite(kept)
            np.testing.assert_array_equal(out["xx"][fin], np.trunc(kept[fin]).astype(np.int32))
        else:
            _bits(out["xx"], kept, repr(rec))


def check_rebuild(rec):
    np.testing.assert_array_equal(rec.out, TCLEAN.ref_indptr(rec.args[0], rec.args[1] != 0))


def check_csr_by_coo(rec):
    p, j, x, ci, cj, cv, m, n = rec.args
    X = SimpleNamespace(p=p, j=j, x=x, Dim=(m, n))
    with np.errstate(all="ignore"):
        r, c, v = TCOO.ref_csr_by_coo(X, ci, cj, cv, rec.fn.startswith("logicaland"))
    np.testing.assert_array_equal(rec.out["row"], r)
    np.testing.assert_array_equal(rec.out["col"], c)
    refpin.exact(rec.out["val"], v, repr(rec))


def check_slice(rec):
    binary = rec.fn.endswith("binary")
    ii, jj = rec.args[:2]
    xx = None if binary else rec.args[2]
    i1, j1 = rec.args[2 + (not binary)], rec.args[3 + (not binary)]
    m, n = rec.args[-2], rec.args[-1]
    for model in (TSLICE.ref_slice_loop(ii, jj, xx, i1, j1), TSLICE.ref_slice(ii, jj, xx, i1, j1, m, n)):
        np.testing.assert_array_equal(rec.out["ii"], model[0])
        np.testing.assert_array_equal(rec.out["jj"], model[1])
        if not binary:
            _bits(rec.out["xx"], model[2], repr(rec))


CHECKS = {"multiply_csr_by_dvec_with_NAs": check_dvec_na, "multiply_csr_by_svec_": check_svec, "multiply_csc_by_dense_": check_csc,
          "logicaland_csc_by_dense_": check_csc, "remove_zero_valued_": check_cleanup, "rebuild_indptr_after_filter": check_rebuild,
          "multiply_csr_by_coo_elemwise": check_csr_by_coo, "logicaland_csr_by_coo_elemwise": check_csr_by_coo,
          "slice_coo_arbitrary_": check_slice}


def checker(fn):
    for prefix, f in CHECKS.items():
        if fn.startswith(prefix):
            return f
    return None


MODELLED = [r for r in RECORDS if checker(r.fn) and r.err is None]


def test_every_model_meets_its_records():
    assert {f for r in MODELLED for f in [checker(r.fn)]} == set(CHECKS.values())
    assert sum(r.fn == "multiply_csr_by_dvec_with_NAs" for r in MODELLED) >= 40


@pytest.mark.parametrize("rec", MODELLED, ids=[f"{n:03d}-{r!r}" for n, r in enumerate(MODELLED)])
def test_model_reproduces_the_reference_run(rec):
    checker(rec.fn)(rec)


# ----------------------------------------------------------------------------- live, other seeds
needs_ref = pytest.mark.skipif(not (Ref.available() or (Ref.sources_present() and Ref.build() and Ref.available())),
                               reason="neither oracle/_ref/libmxref.so nor the reference's sources are here")


def _live(fn, *args):
    rec = refpin.capture(Ref, fn, args, "live")
    assert rec.err is None, rec.err
    checker(fn)(rec)


def lgl(rng, n, na=0.25):
    return rng.choice(np.array([0, 1, NA], dtype=np.int32), size=n, p=[(1 - na) / 2, (1 - na) / 2, na])


@needs_ref
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("op", DM.OPS)
def test_live_dvec_na(op, seed):
    fl = DM.flags(op)
    m, ncols = 30 + 6 * seed, 11
    p, j, x = DM.make_csr(m, ncols, 0.3, 500 + seed, empty_rows=(2,), full_rows=(7,), positive=(op == "^"))
    for L in (m, m // 2 if m % 2 == 0 else m, 1, 7, m * ncols, m + 5):
        v = DM.make_vector(L, op, 510 + seed + L, at=(0, L - 1), share=0.2 if L > 1 else 0.0)
        _live("multiply_csr_by_dvec_with_NAs", p, j, x, v, ncols, *fl, True)
    for flat in (False, True):
        dp, dj, dx, dv, dn = DM.dirty_case(op, flat)
        _live("multiply_csr_by_dvec_with_NAs", dp, dj, dx, dv, dn, *fl, True)
    if op in ("*", "%/%"):
        _live("multiply_csr_by_dvec_with_NAs", p, j, x, DM.make_vector(m, op, 530 + seed, share=0.2), ncols, *fl, False)


@needs_ref
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_live_svec_csc_coo_cleanup_slice(seed):
    rng = np.random.default_rng(600 + seed)
    m, n = 24 + 6 * seed, 9 + seed
    p, j, x = rand_csr(m, n, 0.4, seed=610 + seed, empty_rows=(3,))
    x = x.copy(); x[::19] = np.nan; x[2::7] = np.inf; x[4::9] = 0.0; x[1::23] = DM.NA_REAL      # few NaN * NaN cells: their cap is 5 %
    for L in (m, 6):                    # the routine's precondition: length divides the row count (operators.cpp:3532)
        vi = np.sort(rng.choice(np.arange(1, L + 1), size=max(1, L // 2), replace=False)).astype(np.int32)
        vx = rng.choice(np.array([2.0, -1.5, 0.0, np.inf, -np.inf, DM.NA_REAL, DM.OTHER_NAN]), size=vi.size,
                        p=[0.3, 0.25, 0.1, 0.1, 0.1, 0.1, 0.05])
        for xx in (vx, np.zeros(0)):
            _live("multiply_csr_by_svec_no_NAs", p, j, x, vi, xx, L)
            _live("multiply_csr_by_svec_keep_NAs", p, j, x, vi, xx, n, L)
    # CSC: m columns of n rows
    D = rng.normal(size=(n, m)).round(2); D[rng.random((n, m)) < 0.15] = DM.NA_REAL; D[rng.random((n, m)) < 0.05] = DM.OTHER_NAN
    Di = rng.integers(-3, 4, size=(n, m)).astype(np.int32); Di[rng.random((n, m)) < 0.2] = NA
    for kind, dense in (("numeric", D), ("float32", D.astype(np.float32)), ("integer", Di), ("logical", lgl(rng, n * m).reshape(n, m))):
        _live(f"multiply_csc_by_dense_ignore_NAs_{kind}", p, j, x, np.asfortranarray(dense))
        _live(f"multiply_csc_by_dense_keep_NAs_{kind}", p, j, x, np.asfortranarray(dense))
    _live("logicaland_csc_by_dense_ignore_NAs", p, j, lgl(rng, j.size), np.asfortranarray(lgl(rng, n * m).reshape(n, m)))
    ci, cj = rng.integers(0, m + 2, size=80).astype(np.int32), rng.integers(0, n + 2, size=80).astype(np.int32)
    cv = rng.normal(size=80).round(2); cv[::7] = np.nan; cv[1::9] = 0.0
    _live("multiply_csr_by_coo_elemwise", p, j, x, ci, cj, cv, m, n)
    _live("logicaland_csr_by_coo_elemwise", p, j, lgl(rng, j.size), ci, cj, lgl(rng, 80), m, n)
    xd = rng.choice(np.array([0.0, -0.0, 1.5, -2.0, DM.NA_REAL, DM.OTHER_NAN, np.inf]), size=j.size)
    rr = np.repeat(np.arange(m, dtype=np.int32), np.diff(p))
    for na_rm in (False, True):
        _live("remove_zero_valued_csr_numeric", p, j, xd, na_rm)
        _live("remove_zero_valued_coo_numeric", rr, j, xd, na_rm)
        _live("remove_zero_valued_coo_logical", rr, j, lgl(rng, j.size), na_rm)
        _live("remove_zero_valued_svec_numeric", j + 1, xd, na_rm)
        _live("remove_zero_valued_svec_integer", j + 1, rng.choice(np.array([0, 2, -1, NA], np.int32), size=j.size), na_rm)
        _live("remove_zero_valued_svec_logical", j + 1, lgl(rng, j.size), na_rm)
        rec = refpin.capture(Ref, "remove_zero_valued_csr_logical", (p, j, lgl(rng, j.size), na_rm), "live")
        if "values" not in rec.alias:
            rec.out["values"] = refpin.defined_values(rec.out["values"])
        check_cleanup(rec)
    _live("rebuild_indptr_after_filter", p, lgl(rng, j.size))
    ti, tj = rng.integers(0, m, size=70).astype(np.int32), rng.integers(0, n, size=70).astype(np.int32)
    tx = rng.normal(size=70).round(2)
    i1 = rng.integers(1, m + 1, size=9).astype(np.int32)
    j1 = rng.integers(1, n + 1, size=6).astype(np.int32)
    _live("slice_coo_arbitrary_numeric", ti, tj, tx, i1, j1, False, False, False, False, False, False, m, n)
    _live("slice_coo_arbitrary_logical", ti, tj, lgl(rng, 70), i1, j1, False, False, False, False, False, False, m, n)
    _live("slice_coo_arbitrary_binary", ti, tj, i1, j1, False, False, False, False, False, False, m, n)
    s1, r1 = np.arange(3, 9, dtype=np.int32), np.arange(8, 2, -1).astype(np.int32)
    _live("slice_coo_arbitrary_numeric", ti, tj, tx, s1, s1[:4], False, False, True, True, False, False, m, n)
    _live("slice_coo_arbitrary_numeric", ti, tj, tx, r1, r1[:4], False, False, False, False, True, True, m, n)
