"""The HIP exports (matrixextra_amd/exports.py) against what the reference's own compiled C++ returned for the same
inputs: tests/golden/reference_golden.npz only, nothing outside the repository.  Bars: tests/refpin.py."""
import pytest

import refpin

RECORDS, _META = refpin.load()

# the deviations that DESIGN.md declares on purpose are named in refpin.py (compare_device), shared with the replay
# of the same records through the .Call shim (tests/test_gpu_rshim.py)


@pytest.mark.gpu
@pytest.mark.parametrize("rec", RECORDS, ids=[f"{n:03d}-{r!r}" for n, r in enumerate(RECORDS)])
def test_hip_reproduces_the_reference_run(gpu, rec):
    from matrixextra_amd import exports as G
    assert refpin.has(G, rec.fn), f"matrixextra_amd.exports has no {rec.fn}"
    got, live = refpin.replay(G, rec)
    refpin.compare_device(rec, got, live)
