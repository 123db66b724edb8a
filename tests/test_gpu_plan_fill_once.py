"""The fill classifies every entry of the register-resident chunks once (panel, rank among the chunk's entries of the
panel, per-panel counts) and places it from what it kept; the number of panel bits is a template parameter.  The plan
must stay what test_gpu_plan_build's numpy restatement says, byte for byte, at every panel-bit count (both sides of
each power of two) and with bundles on both sides of a 64-entry chunk, of the 256 entries that stay in registers and
of the 384-step LDS stage."""
import numpy as np
import pytest

from devmem import DevCSR, plan_create
from matrixextra_amd import _lib
from test_gpu_plan_build import assert_plan_equal, csr_from_lengths

K = 4099                                            # prime: K % P != 0 for every P > 1
M = 64 * 9 + 3
BUNDLE_LENS = (0, 1, 63, 64, 65, 255, 256, 257, 384, 385)
PANELS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)


def row_lengths(seed):
    """M rows whose bundles of 8 rows hold exactly one of BUNDLE_LENS entries each: octet 0 stays under the stage
    limit, octet 1 is exactly 384 steps (the largest staged octet), octet 2 is 416 steps (scattered); the rest are
    drawn from the list.  The last bundle has 3 rows."""
    rng = np.random.default_rng(seed)
    nb = -(-M // 8)
    blen = rng.choice(BUNDLE_LENS, size=nb)
    blen[0:8] = (0, 1, 63, 64, 65, 255, 256, 257)
    blen[8:16] = (384, 0, 1, 63, 64, 65, 255, 256)
    blen[16:24] = (385, 257, 256, 1, 0, 384, 64, 65)
    lens = np.zeros(nb * 8, dtype=np.int64)
    for b in range(nb):
        rows = 8 if b * 8 + 8 <= M else M - b * 8
        w = rng.random(rows) * (rng.random(rows) < 0.8)             # some empty rows
        if w.sum() == 0:
            w[0] = 1
        lens[b * 8:b * 8 + rows] = rng.multinomial(blen[b], w / w.sum())
    lens = lens[:M]
    got = np.add.reduceat(lens, np.arange(0, M, 8))
    assert set(got.tolist()) == set(BUNDLE_LENS) and np.array_equal(got, blen)
    return lens


def build_and_compare(p, j, x, P, what):
    A = DevCSR(p, j, x, K)
    plan = plan_create(A, npanels=P)
    try:
        assert_plan_equal(plan, p, j, x, K, P, what)
    finally:
        _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
@pytest.mark.parametrize("P", PANELS)
def test_fill_once_every_panel_bit_count(gpu, P):
    p, j, x = csr_from_lengths(row_lengths(seed=P), K, seed=200 + P)
    build_and_compare(p, j, x, P, f"P={P}")


@pytest.mark.gpu
def test_fill_once_all_entries_in_one_panel(gpu):
    p, j, x = csr_from_lengths(row_lengths(seed=41), K, seed=42)
    for P in PANELS:
        pc = -(-K // P)
        q = P // 2                                                  # every column inside panel q
        jq = (q * pc + j % min(pc, K - q * pc)).astype(np.int32)
        build_and_compare(p, jq, x, P, f"one panel ({q}) P={P}")


@pytest.mark.gpu
def test_fill_once_last_column(gpu):
    """columns K - 1 (and a few others): the last panel is narrower than the rest, K % P != 0"""
    p, j, x = csr_from_lengths(row_lengths(seed=43), K, seed=44)
    jl = np.where(np.arange(j.size) % 5 == 0, j, K - 1).astype(np.int32)
    for P in PANELS:
        assert P == 1 or K % P != 0
        build_and_compare(p, jl, x, P, f"last column P={P}")


@pytest.mark.gpu
def test_fill_once_unsorted_rows(gpu):
    p, j, x = csr_from_lengths(row_lengths(seed=45), K, seed=46, unsorted=True)
    for P in PANELS:
        build_and_compare(p, j, x, P, f"unsorted P={P}")
