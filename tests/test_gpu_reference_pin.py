"""The HIP exports (matrixextra_amd/exports.py) against what the reference's own compiled C++ returned for the same
inputs: tests/golden/reference_golden.npz only, nothing outside the repository.  Bars: tests/refpin.py."""
import numpy as np
import pytest

import refpin

RECORDS, _META = refpin.load()

# ---- deviations that DESIGN.md declares on purpose; each names the records it covers
# remove_zero_valued_svec_numeric: the reference collects the kept values into an IntegerVector (misc.cpp:914), so a
# removal truncates them toward zero.  The device keeps the doubles; `ii` is compared as usual and `xx` against the
# kept input values, whose truncation must be what the reference holds.
SVEC_NUMERIC_KEEPS_DOUBLES = "remove_zero_valued_svec_numeric"


def _svec_numeric(rec, got, live):
    want = rec.out
    if "xx" in rec.alias:                                   # nothing removed: the inputs themselves, no truncation
        return refpin.compare(rec, got, live, device=True)
    refpin.exact(got["ii"], want["ii"], f"{rec!r}[ii]")
    ii, xx = rec.args[0], rec.args[1]
    keep = xx != 0                                          # only zeros leave, with or without na.rm
    np.testing.assert_array_equal(ii[keep], want["ii"])
    kept = xx[keep]
    refpin.exact(got["xx"], kept, f"{rec!r}[xx]")
    fin = np.isfinite(kept)
    np.testing.assert_array_equal(np.trunc(kept[fin]).astype(np.int32), want["xx"][fin])


@pytest.mark.gpu
@pytest.mark.parametrize("rec", RECORDS, ids=[f"{n:03d}-{r!r}" for n, r in enumerate(RECORDS)])
def test_hip_reproduces_the_reference_run(gpu, rec):
    from matrixextra_amd import exports as G
    assert refpin.has(G, rec.fn), f"matrixextra_amd.exports has no {rec.fn}"
    got, live = refpin.replay(G, rec)
    if rec.fn == SVEC_NUMERIC_KEEPS_DOUBLES and rec.err is None and not isinstance(got, Exception):
        return _svec_numeric(rec, got, live)
    refpin.compare(rec, got, live, device=True)
