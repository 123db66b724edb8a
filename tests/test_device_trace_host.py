"""matrixextra_amd/device.py against tests/golden/device_call_trace.json: every wrapper, over the recording fake of
tests/device_trace.py, makes the library calls, the allocations and the results that the record holds, and refuses
what it refused with the same exception and words.  No library and no device is needed."""
import json
import os

import pytest

import device_trace as T

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_call_trace.json")) as f:
    RECORD = json.load(f)
CASES, REFUSALS = T.cases(), T.refusals()


def test_the_record_and_the_cases_name_the_same_things():
    assert sorted(RECORD["cases"]) == sorted(CASES)
    assert sorted(RECORD["refusals"]) == sorted(REFUSALS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_trace(name):
    got = json.loads(json.dumps(T.run_case(CASES[name])))       # tuples become lists, as in the file
    want = RECORD["cases"][name]
    assert got["calls"] == want["calls"]
    assert got["allocations"] == want["allocations"]
    assert got == want


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name):
    assert T.run_refusal(REFUSALS[name]) == RECORD["refusals"][name]
