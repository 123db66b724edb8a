"""The numpy model of the vector-valued CSR assignment (tests/assign_vec_model.py) against the record of what the
reference's own compiled routines returned (tests/golden/assign_vec_golden.npz), and against hand-written
expectations where the reference is not the yardstick: the two defects of set_single_row_to_svec's fast path and the
empty ii it divides by zero on.  No GPU, no library."""
import numpy as np
import pytest

import assign_vec_model as VM

RECORDS, META = VM.load()
I32 = lambda *a: np.array(a, dtype=np.int32)        # noqa: E731


def same(got, want, what=""):
    for a, b, k in zip(got[:2], want[:2], ("indptr", "indices")):
        assert np.array_equal(a, b), f"{what}: {k}"
    assert np.array_equal(VM.bits(got[2]), VM.bits(want[2])), f"{what}: values"


def sorted_rows(t):
    return (t[0],) + VM.sort_rows(*t)


def test_the_record_is_what_the_generator_says():
    assert {r["name"] for r in RECORDS} == set(VM.ORDER)
    n_sorted = sum(r["sorted"] for r in RECORDS)
    assert n_sorted == META["sorted_records"] and len(RECORDS) - n_sorted == META["shuffled_records"]
    assert all(r["label"].startswith("shuffled:") for r in RECORDS if not r["sorted"])
    assert "src/assignment.cpp:771-1133" in META["source"] and "-O" in META["flags"]
    vals = np.concatenate([VM.bits(r["args"]["vec"] if "vec" in r["args"] else r["args"]["xx"]) for r in RECORDS])
    for special in (0.0, -0.0, VM.NA_REAL, VM.OTHER_NAN):
        assert (vals == VM.bits(np.array([special]))[0]).any(), special
    assert any(r["args"]["ii"].size == 0 for r in RECORDS if r["name"] == "set_single_col_to_svec")
    assert all(r["args"]["ii"].size > 0 for r in RECORDS if r["name"] == "set_single_row_to_svec")
    assert any(np.any(np.diff(r["args"]["ii"]) < 0) for r in RECORDS if r["name"] == "set_single_row_to_svec")


@pytest.mark.parametrize("name", sorted(VM.ORDER))
def test_model_equals_the_reference(name):
    n = aliased = 0
    for r in RECORDS:
        if r["name"] != name:
            continue
        got = VM.run(name, r["p"], r["j"], r["x"], r["args"])
        want = (r["out_p"], r["out_j"], r["out_x"])
        if r["sorted"]:
            same(got, want, r["label"])
            assert VM.alias_rule(name, r["p"], r["j"], r["args"]) == r["alias"], r["label"]
            aliased += r["alias"] == (1, 1, 0)
        else:
            sj, sx = VM.sort_rows(r["p"], r["j"], r["x"])
            if "col" in r["args"]:                    # the column routes work on a sorted copy
                got = VM.run(name, r["p"], sj, sx, r["args"])
            same(sorted_rows(got), sorted_rows(want), r["label"])
        n += 1
    assert n >= 20
    assert (aliased > 0) == (name != "set_single_col_to_svec")


def test_examples_of_the_contract():
    # a dense vector's zeros are stored positions like any other
    p, j, x = I32(0, 1, 2), I32(1, 0), np.array([1.0, 2.0])
    got = VM.run("set_single_row_to_rowvec", p, j, x, dict(ncols=6, row=0, vec=np.array([0.0, 7.0, VM.OTHER_NAN])))
    same(got, (I32(0, 6, 7), I32(0, 1, 2, 3, 4, 5, 0), np.array([0, 7, VM.OTHER_NAN, 0, 7, VM.OTHER_NAN, 2.0])))
    # an explicit zero of a sparse vector is written; an unstored position drops the column
    p, j, x = I32(0, 2, 3, 3, 5), I32(0, 3, 3, 1, 3), np.arange(1.0, 6.0)
    got = VM.run("set_single_col_to_svec", p, j, x, dict(ncols=5, col=3, ii=I32(0), xx=np.array([0.0]), length=2))
    same(got, (I32(0, 2, 2, 3, 4), I32(0, 3, 3, 1), np.array([1.0, 0.0, 0.0, 4.0])))
    got = VM.run("set_single_col_to_svec", p, j, x, dict(ncols=5, col=3, ii=I32(), xx=np.zeros(0), length=4))
    same(got, (I32(0, 1, 1, 1, 2), I32(0, 1), np.array([1.0, 4.0])))
    # the inserted entry lands at its ascending place: below all, between, above all, into an empty row
    p, j, x = I32(0, 2, 4, 6, 6), I32(3, 4, 0, 4, 0, 1, ), np.arange(1.0, 7.0)
    got = VM.run("set_single_col_to_colvec", p, j, x, dict(ncols=5, col=2, vec=np.array([VM.NA_REAL, -0.0])))
    same(got, (I32(0, 3, 6, 9, 10), I32(2, 3, 4, 0, 2, 4, 0, 1, 2, 2),
               np.array([VM.NA_REAL, 1, 2, 3, -0.0, 4, 5, 6, VM.NA_REAL, -0.0])))


def test_the_defects_of_the_fast_path_are_not_the_model():
    # n_repeats > 1, a row shorter than the recycled pattern (src/assignment.cpp:949-959): the reference returns the
    # input structure with values [50, 50], overwriting row 1; the model replaces row 0 and leaves row 1 alone
    p, j, x = I32(0, 1, 2), I32(1, 0), np.array([1.0, 2.0])
    args = dict(ncols=6, row=0, ii=I32(1), xx=np.array([50.0]), length=3)
    same(VM.run("set_single_row_to_svec", p, j, x, args), (I32(0, 2, 3), I32(1, 4, 0), np.array([50.0, 50.0, 2.0])))
    assert VM.alias_rule("set_single_row_to_svec", p, j, args) == (0, 0, 0)
    # n_repeats = 1, a row twice as long as ii (:942-947 reads ii[2], ii[3])
    p, j, x = I32(0, 4), I32(0, 2, 3, 5), np.arange(1.0, 5.0)
    args = dict(ncols=6, row=0, ii=I32(0, 2), xx=np.array([7.0, 8.0]), length=6)
    same(VM.run("set_single_row_to_svec", p, j, x, args), (I32(0, 2), I32(0, 2), np.array([7.0, 8.0])))
    assert VM.alias_rule("set_single_row_to_svec", p, j, args) == (0, 0, 0)
    # an empty ii (the reference divides by zero, :939) empties the row
    p, j, x = I32(0, 2, 3), I32(0, 4, 2), np.array([1.0, 2.0, 3.0])
    args = dict(ncols=6, row=0, ii=I32(), xx=np.zeros(0), length=3)
    same(VM.run("set_single_row_to_svec", p, j, x, args), (I32(0, 0, 1), I32(2), np.array([3.0])))
    assert VM.alias_rule("set_single_row_to_svec", p, j, args) == (0, 0, 0)
    # the fast path proper: equal lengths and equal indices, recycled
    p, j, x = I32(0, 4, 5), I32(1, 2, 4, 5, 0), np.arange(1.0, 6.0)
    args = dict(ncols=6, row=0, ii=I32(1, 2), xx=np.array([7.0, 8.0]), length=3)
    same(VM.run("set_single_row_to_svec", p, j, x, args), (p, j, np.array([7.0, 8.0, 7.0, 8.0, 5.0])))
    assert VM.alias_rule("set_single_row_to_svec", p, j, args) == (1, 1, 0)
