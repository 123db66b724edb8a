"""The numpy model of the COO sort (tests/coo_sort_model.py) against a hand-worked case, against the reference-run
fixture tests/golden/coo_sort_golden.npz, and live against the reference's own compiled sort_coo_indices_* on a wider
seeded sweep when oracle/_ref/libmxref.so is there.  No GPU."""
import os

import numpy as np
import pytest

import coo_sort_model as CM
from oracle import ref as Ref

RECORDS, META = CM.load()
needs_ref = pytest.mark.skipif(not (Ref.available() or (Ref.sources_present() and Ref.build() and Ref.available())),
                               reason="neither oracle/_ref/libmxref.so nor the reference's sources are here")


def test_hand_worked_case():
    """(2,1) (0,3) (2,0) (0,3) with values a b c d: row 0 first, its two (0,3) entries in input order b, d; then row 2
    by column: (2,0) c, (2,1) a."""
    a, b, c, d = 1.5, -2.0, 0.25, 7.0
    i, j, x = CM.model([2, 0, 2, 0], [1, 3, 0, 3], np.array([a, b, c, d]))
    assert i.tolist() == [0, 0, 2, 2] and j.tolist() == [3, 3, 0, 1] and x.tolist() == [b, d, c, a]
    i, j, x = CM.model([2, 0, 2, 0], [1, 3, 0, 3])
    assert i.tolist() == [0, 0, 2, 2] and j.tolist() == [3, 3, 0, 1] and x is None


def test_fixture_is_small_and_covers_every_kind():
    assert os.path.getsize(CM.PATH) < 100 * 1024
    assert META["flags"] and int(META["seed"]) > 0
    for kind in CM.KINDS:
        mine = [r for r in RECORDS if r["kind"] == kind]
        sizes = {r["i"].size for r in mine}
        assert {0, 1} <= sizes
        assert any(CM.has_repeats(r["i"], r["j"]) for r in mine) and any(not CM.has_repeats(r["i"], r["j"]) for r in mine)
        assert all((r["x"] is None) == (kind == "binary") for r in mine)
        assert all(r["x"] is None or r["x"].dtype == CM.VALUE_DTYPE[kind] for r in mine)
        big = max(mine, key=lambda r: r["i"].size)
        assert not np.array_equal(big["i"], big["ri"])                       # the reference did move something


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: f"{r['kind']}-{r['label']}")
def test_model_matches_the_fixture(rec):
    inp = (rec["i"], rec["j"], rec["x"])
    got = CM.model(*inp)
    CM.assert_matches_reference(got, (rec["ri"], rec["rj"], rec["rx"]), f"{rec['kind']} {rec['label']}")
    CM.assert_equals_model(got, inp, rec["label"])
    if rec["label"] == "sorted_already":
        CM.assert_matches_reference(inp, (rec["ri"], rec["rj"], rec["rx"]), "sorted input stays")
    if rec["x"] is not None and CM.has_repeats(rec["i"], rec["j"]):
        # the model's order inside a cell is input order: tag every entry with its position and look at the tags
        tag = np.arange(rec["i"].size, dtype=np.float64)
        si, sj, st = CM.model(rec["i"], rec["j"], tag)
        same = (si[1:] == si[:-1]) & (sj[1:] == sj[:-1])
        assert same.any() and np.all(st[1:][same] > st[:-1][same])


@needs_ref
@pytest.mark.parametrize("kind", CM.KINDS)
def test_model_matches_the_reference_live(kind):
    rng = np.random.default_rng(977)
    shapes = [(1, 1), (1, 50), (50, 1), (13, 17), (300, 300), (257, 65537), (65537, 2)]
    for nrow, ncol in shapes:
        for n in sorted({0, 1, min(nrow * ncol, 2), min(nrow * ncol, 64), min(nrow * ncol, 700)}):
            i, j = CM.unique_cells(nrow, ncol, n, rng)
            inp = (i, j, CM.values_for(kind, n, rng))
            got = CM.model(*inp)
            CM.assert_matches_reference(got, CM.run(Ref, kind, *inp), f"{kind} unique {nrow}x{ncol} n={n}")
        for n in (5, 90, 400):
            i, j = CM.repeated_cells(min(nrow, 6), min(ncol, 7), n, rng)
            inp = (i, j, CM.values_for(kind, n, rng))
            got = CM.model(*inp)
            CM.assert_matches_reference(got, CM.run(Ref, kind, *inp), f"{kind} repeats {nrow}x{ncol} n={n}")
            CM.assert_equals_model(got, inp, "stable")


@needs_ref
def test_fixture_is_what_the_reference_gives_now():
    assert META["flags"] == Ref.compile_flags()
    for rec in RECORDS:
        if not CM.has_repeats(rec["i"], rec["j"]):          # unique cells: every bit is fixed
            ri, rj, rx = CM.run(Ref, rec["kind"], rec["i"], rec["j"], rec["x"])
            assert np.array_equal(ri, rec["ri"]) and np.array_equal(rj, rec["rj"])
            assert rx is None or np.array_equal(CM.bits(rx), CM.bits(rec["rx"]))
