"""The numpy model of `matrix * sparseVector` and of the COO * dense gather (tests/dense_svec_model.py) against
hand-worked cases, against the reference-run fixture tests/golden/dense_svec_golden.npz, and live against the
reference's own compiled code on the full grid of shapes when oracle/_ref/libmxref.so is there.  No GPU.

Bars: bit for bit (refpin.exact, and NaN payloads too through dense_svec_model.same), apart from NaN * NaN products
(at most 5 % of a case).  model(as_reference=True) restates the reference as it is, deviations 2 and 5 of DESIGN.md
§4.15 included; model() is what the device computes, and the two differ at the named cells only."""
import os

import numpy as np
import pytest

import dense_svec_model as M
import refpin
from oracle import ref as Ref

RECORDS, META = refpin.load(M.PATH)
SVEC = [r for r in RECORDS if r.fn in M.KIND_OF_FN]
COO = [r for r in RECORDS if r.fn in M.COO_KIND_OF_FN]
needs_ref = pytest.mark.skipif(not (Ref.available() or (Ref.sources_present() and Ref.build() and Ref.available())),
                               reason="neither oracle/_ref/libmxref.so nor the reference's sources are here")


def _args(rec):
    return rec.args[0], rec.args[1], rec.args[2], int(rec.args[3]), bool(rec.args[4])


def test_routes_in_the_reference_order():
    assert M.route(63, 1, 63) == "A"                        # one column: the tie with route B goes to A
    assert M.route(65, 2, 130) == "A" and M.route(65, 2, 65) == "B" and M.route(65, 2, 13) == "C"
    assert M.route(65, 2, 7) == "D" and M.route(65, 2, 68) == "D" and M.route(1, 64, 1) == "B"


def test_hand_worked_routes():
    X = np.asfortranarray(np.array([[1.0, 2.0], [0.0, np.inf], [np.nan, 4.0], [5.0, 6.0]]))
    ii, xx = np.array([1, 2], dtype=np.int32), np.array([3.0, -1.0])
    res, _ = M.model("numeric", X, ii, xx, 2, False)       # route C without NAs: daxpy, so -1 * 0 is +0.0
    assert res["indptr"].tolist() == [0, 2, 4, 6, 8] and res["indices"].tolist() == [0, 1] * 4
    assert M.bits(res["values"])[2] == 0 and res["values"][3] == -np.inf and np.isnan(res["values"][4])
    res, _ = M.model("numeric", X, ii[:1], xx[:1], 4, False)      # route B: row 0 only
    assert res["indptr"].tolist() == [0, 2, 2, 2, 2] and res["values"].tolist() == [3.0, 6.0]
    res, _ = M.model("numeric", X, ii[:1], xx[:1], 4, True)       # route B keeping NAs: Inf becomes C's NAN, NaN stays
    assert res["indptr"].tolist() == [0, 2, 3, 4, 4] and res["indices"].tolist() == [0, 1, 1, 0]
    assert M.bits(res["values"][2:3])[0] == M.bits(np.array([M.C_NAN]))[0]
    res, _ = M.model("numeric", X, np.array([2, 8], dtype=np.int32), np.array([2.0, 10.0]), 8, True)   # route A
    assert res["X_dense"][1, 0] == 0.0 and res["X_dense"][3, 1] == 60.0 and np.isnan(res["X_dense"][2, 0])
    res, _ = M.model("numeric", X, np.array([1], dtype=np.int32), np.array([2.0]), 3, False)           # route D: cells 0, 3, 6
    assert res["X_dense"].reshape(-1, order="F").tolist() == [2.0, 0, 0, 10.0, 0, 0, 8.0, 0]
    assert M.overruns(4, 2, np.array([3]), 3) and not M.overruns(4, 2, np.array([1, 2]), 3)


def test_fixture_is_small_and_covers_the_ground():
    assert os.path.getsize(M.PATH) < 128 * 1024
    assert META["flags"] and int(META["seed"]) > 0
    seen = set()
    for r in SVEC:
        X, ii, xx, length, keep = _args(r)
        assert not M.overruns(*X.shape, ii, length), f"{r!r}: deviation 1 input in the fixture"
        assert ii.size == 0 or (ii.min() >= 1 and ii.max() <= length and np.all(np.diff(ii) > 0))
        seen.add((M.KIND_OF_FN[r.fn], M.route(*X.shape, length), keep))
    assert seen == {(k, rt, kp) for k in M.KINDS for rt in "ABCD" for kp in (False, True)}
    assert {r.fn for r in COO} == set(M.COO_FN.values())
    assert {r.args[1].size for r in COO} == {0, 1, 65, 4099}
    assert any(r.args[0].shape[1] == 1 and r.args[3] == r.args[0].shape[0] and "X_dense" in r.out for r in SVEC)
    values = np.concatenate([r.args[2] for r in SVEC])
    assert np.isinf(values).any() and np.isnan(values).any() and (values == 0).any() and (values == -1).any()


@pytest.mark.parametrize("rec", SVEC, ids=[repr(r) for r in SVEC])
def test_model_matches_the_fixture(rec):
    X, ii, xx, length, keep = _args(rec)
    kind = M.KIND_OF_FN[rec.fn]
    want, both = M.model(kind, X, ii, xx, length, keep, as_reference=True)
    M.compare_results(want, rec.out, both, repr(rec))
    for key, w in rec.out.items():                          # and under the shared bar
        refpin.exact(want[key], w, f"{rec!r}[{key}]")
    # the device's model differs from the reference at the named deviations only
    M.compare_svec(rec.fn, rec.args, M.model(kind, X, ii, xx, length, keep)[0], rec.out, repr(rec))


def test_named_deviations_are_in_the_fixture():
    dev2 = [r for r in SVEC if (lambda n: n is not None and n.any())(M.int_na_tail_cells(M.KIND_OF_FN[r.fn], *_args(r)[:2], *_args(r)[3:]))]
    dev5 = [r for r in SVEC if M.recycles_under_keep(*r.args[0].shape, r.args[1].size, int(r.args[3]), bool(r.args[4]))]
    assert {M.KIND_OF_FN[r.fn] for r in dev2} == {"integer", "logical"}
    assert {M.KIND_OF_FN[r.fn] for r in dev5} == set(M.KINDS)
    for r in dev2:
        named = M.int_na_tail_cells(M.KIND_OF_FN[r.fn], *_args(r)[:2], *_args(r)[3:])
        assert np.all(r.out["values"][named] == -2147483648.0)
        mine = M.model(M.KIND_OF_FN[r.fn], *_args(r))[0]["values"]
        assert not (mine == -2147483648.0).any()


@pytest.mark.parametrize("rec", COO, ids=[repr(r) for r in COO])
def test_coo_model_matches_the_fixture(rec):
    X, ii, jj, xx = rec.args
    val, both = M.coo_model(M.COO_KIND_OF_FN[rec.fn], X, ii, jj, xx)
    M.compare_coo(rec.args, rec.fn, dict(row=ii, col=jj, val=val), rec.out, repr(rec))
    refpin.exact(val, rec.out["val"], repr(rec))
    assert not rec.alias                                    # the reference copies row and col (:763-769)


@needs_ref
@pytest.mark.parametrize("kind", M.KINDS)
def test_model_matches_the_reference_live(kind):
    """The full grid of the issue: every shape at the tile's edges, every length whose route holds, every pattern."""
    n = 0
    for nrows in M.NROWS:
        for ncols in M.NCOLS:
            for length, rt in M.lengths_for(nrows, ncols):
                for keep in (False, True):
                    pattern = M.PATTERNS[n % len(M.PATTERNS)]
                    X, ii, xx = M.svec_case(kind, nrows, ncols, length, pattern, 5100 + n)
                    n += 1
                    assert not M.overruns(nrows, ncols, ii, length)
                    got = getattr(Ref, M.SVEC_FN[kind])(X, ii, xx, length, int(keep))
                    want, both = M.model(kind, X, ii, xx, length, keep, as_reference=True)
                    M.compare_results(want, got, both, f"{kind} {nrows}x{ncols} L{length}{rt} {pattern} keep={keep}")
    assert n > 200


@needs_ref
def test_fixture_is_what_the_reference_gives_now():
    assert META["flags"] == Ref.compile_flags()
    for rec in RECORDS:
        got, live = refpin.replay(Ref, rec)
        refpin.compare(rec, got, live, device=False)
