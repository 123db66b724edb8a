"""tests/assign_model.py against tests/golden/assign_golden.npz: the plain model of DESIGN.md 4.16 reproduces what the
reference's own compiled set_* routines (src/assignment.cpp) returned, bit for bit, on every record with sorted
rows, and the alias rule names the vectors the reference returned as they came in."""
import collections

import numpy as np
import pytest

import assign_model as AM

RECORDS, META = AM.load()


def test_the_golden_covers_every_export_and_every_alias_branch():
    by_name = collections.defaultdict(set)
    for r in RECORDS:
        by_name[r["name"]].add(r["alias"])
    assert set(by_name) == set(AM.ORDER) and len(AM.ORDER) == 22
    for name, seen in by_name.items():
        if name.endswith("_smat") or name in AM.NEVER_ALIAS:
            assert seen == {(0, 0, 0)}, name
        else:
            assert seen == {(0, 0, 0), (1, 1, 1) if name.endswith("_to_zero") else (1, 1, 0)}, name
    consts = {int(AM.bits(r["args"]["val"])[0]) for r in RECORDS if "val" in r["args"]}
    assert consts == {int(AM.bits(2.5)[0]), 0x7FF00000000007A2, int(AM.bits(AM.OTHER_NAN)[0])}
    assert any(r["j"].size == 0 for r in RECORDS) and sum(not r["sorted"] for r in RECORDS) >= 4
    assert "-O2" in META["flags"] and META["seed"] > 0


@pytest.mark.parametrize("name", sorted(AM.ORDER))
def test_the_model_reproduces_the_reference(name):
    n = 0
    for r in RECORDS:
        if r["name"] != name or not r["sorted"]:
            continue
        p, j, x = AM.run(name, r["p"], r["j"], r["x"], r["args"])
        assert np.array_equal(p, r["out_p"]) and np.array_equal(j, r["out_j"]), r["label"]
        assert np.array_equal(AM.bits(x), AM.bits(r["out_x"])), r["label"]
        assert AM.alias_rule(name, r["p"], p, r["j"].size) == r["alias"], r["label"]
        n += 1
    assert n >= 5


def test_unsorted_records_agree_with_the_model_after_sorting_rows():
    """The reference sorts the selected rows of its inputs in place; the device works on a sorted copy.  Both give the
    model's result on the sorted input once every row of the reference's output is sorted."""
    for r in RECORDS:
        if r["sorted"]:
            continue
        sj, sx = AM.sort_rows(r["p"], r["j"], r["x"])
        p, j, x = AM.run(r["name"], r["p"], sj, sx, r["args"])
        oj, ox = AM.sort_rows(r["out_p"], r["out_j"], r["out_x"])
        assert np.array_equal(p, r["out_p"]) and np.array_equal(j, oj) and np.array_equal(AM.bits(x), AM.bits(ox)), \
            (r["name"], r["label"])


def test_the_model_on_a_hand_made_case():
    p, j, x = np.array([0, 2, 2, 4]), np.array([1, 3, 0, 3]), np.array([1.0, 2.0, 3.0, 4.0])
    q, k, y = AM.assign_scalar(p, j, x, 5, np.array([2, 1]), np.array([3, 0]), 0.0)
    assert q.tolist() == [0, 2, 2, 2] and k.tolist() == [1, 3] and y.tolist() == [1.0, 2.0]
    q, k, y = AM.assign_scalar(p, j, x, 5, np.array([2, 1]), np.array([3, 2]), 7.0)
    assert q.tolist() == [0, 2, 4, 7] and k.tolist() == [1, 3, 2, 3, 0, 2, 3]
    assert y.tolist() == [1.0, 2.0, 7.0, 7.0, 3.0, 7.0, 7.0]
    q, k, y = AM.replace_rows(p, j, x, [2, 0], np.array([0, 0, 1]), np.array([4]), np.array([9.0]))
    assert q.tolist() == [0, 1, 1, 1] and k.tolist() == [4] and y.tolist() == [9.0]
