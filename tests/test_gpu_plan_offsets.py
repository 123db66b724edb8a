"""Octet offsets without a scan: the sizing pass writes the steps of every octet and the sum of every tile of T octets
(T = 32 up to 4096 tiles, a larger multiple of 32 beyond); a fill workgroup adds up the tile sums in front of its tile
and the steps in front of it inside the tile, the host adds the tile sums up to the step total.  The plan must stay
what test_gpu_plan_build's numpy restatement says, byte for byte, on both sides of a tile, with more than 4096 x 32
octets, and when one plan object is rebuilt for matrices of different sizes.  AUTO's decisions (pad rule, first-call
growth) are taken from the same sums."""
import numpy as np
import pytest
import scipy.sparse as sp

from devmem import DevCSR, last_kernel, plan_create, spmm_guarded
from matrixextra_amd import _lib
from test_gpu_plan_build import PLANNED, ROWWAVE, _auto_expect, assert_plan_equal, csr_from_lengths

K = 4099


def short_rows(noct, seed):
    """noct octets, the last one incomplete; row lengths 0..5"""
    m = noct * 64 - 5
    lens = np.random.default_rng(seed).integers(0, 6, size=m)
    return csr_from_lengths(lens, K, seed=seed + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("noct", [1, 31, 32, 33, 64, 65, 32 * 17 + 5])
def test_offsets_both_sides_of_a_tile(gpu, noct):
    p, j, x = short_rows(noct, seed=noct)
    assert -(-(p.size - 1) // 64) == noct
    A = DevCSR(p, j, x, K)
    plan = plan_create(A, npanels=8)
    try:
        assert_plan_equal(plan, p, j, x, K, 8, f"noct={noct}")
    finally:
        _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
def test_offsets_more_than_4096_tiles_of_32_octets(gpu):
    m = 64 * (131072 + 33) + 7
    assert -(-m // 64) > 4096 * 32
    lens = np.random.default_rng(5).integers(0, 2, size=m)
    p, j, x = csr_from_lengths(lens, K, seed=6)
    A = DevCSR(p, j, x, K)
    plan = plan_create(A, npanels=3)
    try:
        assert_plan_equal(plan, p, j, x, K, 3, f"m={m}")
    finally:
        _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
def test_offsets_three_builds_into_one_plan(gpu):
    small = short_rows(3, seed=21)
    large = short_rows(32 * 9 + 1, seed=23)
    plan = None
    try:
        for step, (p, j, x) in enumerate((small, large, small)):
            A = DevCSR(p, j, x, K)
            plan = plan_create(A, npanels=8, plan=plan)
            assert_plan_equal(plan, p, j, x, K, 8, f"build {step} (m={p.size - 1})")
    finally:
        if plan is not None:
            _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
def test_auto_pad_rule_rejects_then_accepts(gpu):
    """test_auto_lognormal_rows_both_sides_of_the_pad_rule the other way round: with no workspace yet, the matrix the
    pad rule rejects comes first (nothing is written, the repack is skipped, the row-wave kernel runs), then the one
    it accepts has to grow the plan's buffers and fill again.  C is exact (integer data)."""
    lib = _lib.load()
    lib.mxd_release_workspaces()
    Kc, n, m = 70_001, 16, (1 << 20) + 37
    rng = np.random.default_rng(11)
    cases = {}
    for sigma, expect in ((0.5, PLANNED), (1.3, ROWWAVE)):           # drawn in that test's order: the same matrices
        lens = np.maximum(0, np.round(rng.lognormal(np.log(8), sigma, size=m))).astype(np.int64)
        cases[sigma] = (csr_from_lengths(lens, Kc, seed=int(sigma * 10)), expect)
    L = np.random.default_rng(5).integers(-16, 17, size=(Kc, n)).astype(np.int64)
    B = L.astype(np.float64) / 16
    for sigma in (1.3, 0.5):
        (p, j, x), expect = cases[sigma]
        assert _auto_expect(p) == expect, sigma
        k = (x * 8).astype(np.int64)
        ref = (sp.csr_matrix((k, j, p), shape=(m, Kc)) @ L) / 128.0
        A = DevCSR(p, j, x, Kc)
        for colmajor in (True, False):
            got, err = spmm_guarded(A, B, colmajor, algo=0, rows_sorted=True)
            assert err is None, err
            assert last_kernel() == expect, (sigma, last_kernel())
            np.testing.assert_array_equal(got, ref, err_msg=f"AUTO sigma={sigma} colmajor={colmajor}")
