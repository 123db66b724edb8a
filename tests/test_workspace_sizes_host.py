"""Every mxd_*_workspace_bytes function returns what it returned before the workspace layouts became one struct per
kernel family (csrc/mx_workspace.h): callers allocate these bytes, so no layout may move them.  The record,
tests/golden/workspace_sizes.json, was taken once from the earlier build (tests/golden/make_workspace_sizes.py) and is
never regenerated from the code under test.  No device is needed: the functions are host arithmetic."""
import json
import os

import pytest

from matrixextra_amd import _lib

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")) as f:
    RECORD = json.load(f)


def test_every_size_function_is_recorded():
    declared = {n for n in _lib.declared_symbols() if n.startswith("mxd_") and n.endswith("_workspace_bytes")}
    assert declared == set(RECORD) and len(declared) >= 20


@pytest.mark.parametrize("name", sorted(RECORD))
def test_sizes_are_those_of_the_record(name):
    fn = getattr(_lib.load(), name)
    calls = RECORD[name]
    assert len(calls) >= 1
    wrong = [(args, fn(*args), want) for *args, want in calls if fn(*args) != want]
    assert not wrong, f"{name}: {len(wrong)} of {len(calls)} sizes differ, first (args, got, recorded): {wrong[0]}"
