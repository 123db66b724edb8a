"""The planned kernel's plan, byte for byte.

The plan layout is restated here in numpy from its documented rules (spmm_plan.hip, "v3 planned panel sweep" and "Plan
construction"):
  * rows are cut into bundles of 8 and octets of 8 bundles (64 rows); column panels are ceil(K / P) columns wide,
    the last one takes the rest;
  * inside a bundle the entries are ordered by panel, and inside a panel by CSR storage order; entry = column |
    (row inside the bundle << 27), value;
  * an octet is as long as its longest bundle rounded up to 32 steps; step t of bundle g lands in slot
    (oct_off + (t & ~7)) * 8 + g * 8 + (t & 7); steps past a bundle's end are no-op entries (column K, the bundle's
    last row, value 0), and 512 such slots (row 0) follow the last octet;
  * step_off[oct * P + q] = oct_off + (mean over the 8 bundles of where panel q starts, rounded down; 0 for q = 0),
    step_off[noct * P] = the step total.
Every device plan must equal it exactly, whichever path the fill takes (staged in LDS, or scattered for octets too long
for the stage), and whatever the plan object held before.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from devmem import DevCSR, last_kernel, plan_create, spmm_guarded
from matrixextra_amd import _lib
from matrixextra_amd._lib import check

ROW_SHIFT = 27
TAIL = 512
PLANNED, ROWWAVE = "spmm_plan_kernel", "spmm_rowwave_kernel"


def plan_model(p, j, x, K, P):
    """(step_off, pcol, pval, total steps) of the plan of CSR (p, j, x) with K columns and P panels."""
    p = p.astype(np.int64)
    m, nnz = p.size - 1, int(p[-1])
    noct = -(-m // 64)
    nb = noct * 8
    pc = -(-max(K, 1) // P)
    b_lo = p[np.minimum(np.arange(nb) * 8, m)]
    b_hi = p[np.minimum(np.arange(nb) * 8 + 8, m)]
    blen = b_hi - b_lo
    steps = (blen.reshape(noct, 8).max(axis=1) + 31) // 32 * 32
    oct_off = np.zeros(noct + 1, dtype=np.int64)
    np.cumsum(steps, out=oct_off[1:])
    total = int(oct_off[-1])

    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(p))
    bundle, lrow = rows // 8, rows % 8
    pan = np.minimum(j.astype(np.int64) // pc, P - 1)
    order = np.argsort(bundle * P + pan, kind="stable")          # a bundle's entries stay at [b_lo, b_hi)
    t = np.empty(nnz, dtype=np.int64)
    t[order] = np.arange(nnz, dtype=np.int64) - b_lo[bundle[order]]

    def slot(b, tt):
        return (oct_off[b // 8] + (tt & ~7)) * 8 + (b % 8) * 8 + (tt & 7)

    pcol = np.full(total * 8 + TAIL, K, dtype=np.int32)
    pval = np.zeros(total * 8 + TAIL, dtype=np.float64)
    pcol[slot(bundle, t)] = (j.astype(np.int64) | (lrow << ROW_SHIFT)).astype(np.int32)
    pval[slot(bundle, t)] = x
    # padding: steps blen..steps_oct-1 of every bundle, on the bundle's last row
    npad = np.repeat(steps, 8) - blen
    pb = np.repeat(np.arange(nb, dtype=np.int64), npad)
    first = np.repeat(np.cumsum(npad) - npad, npad)
    pt = blen[pb] + np.arange(pb.size, dtype=np.int64) - first
    last_row = np.where(blen > 0, rows[np.maximum(b_hi - 1, 0)] % 8 if nnz else 0, 0)
    pcol[slot(pb, pt)] = (K | (last_row[pb] << ROW_SHIFT)).astype(np.int32)

    counts = np.bincount(bundle * P + pan, minlength=nb * P).reshape(nb, P)
    bpo = np.cumsum(counts, axis=1) - counts
    mean = bpo.reshape(noct, 8, P).sum(axis=1) // 8
    mean[:, 0] = 0
    step_off = np.append((oct_off[:-1, None] + mean).reshape(-1), total).astype(np.int32)
    return step_off, pcol, pval, total


def device_plan(plan, m):
    lib = _lib.load()
    P, padded = C.c_int(0), C.c_int64(0)
    check(lib.mxd_spmm_plan_info(plan, C.byref(P), C.byref(padded)))
    noct = -(-m // 64)
    step_off = np.empty(noct * P.value + 1, dtype=np.int32)
    pcol = np.empty(padded.value + TAIL, dtype=np.int32)
    pval = np.empty(padded.value + TAIL, dtype=np.float64)
    check(lib.mxd_spmm_plan_copy_to_host(plan, step_off.ctypes.data_as(C.c_void_p), pcol.ctypes.data_as(C.c_void_p),
                                         pval.ctypes.data_as(C.c_void_p), None))
    return P.value, step_off, pcol, pval


def assert_plan_equal(plan, p, j, x, K, P, what):
    """P = None: the panel count the plan chose."""
    Pd, d_step_off, d_pcol, d_pval = device_plan(plan, p.size - 1)
    assert P is None or Pd == P, what
    step_off, pcol, pval, total = plan_model(p, j, x, K, Pd)
    assert d_pcol.size == pcol.size, f"{what}: {d_pcol.size - TAIL} slots, expected {total * 8}"
    np.testing.assert_array_equal(d_step_off, step_off, err_msg=f"{what}: step_off")
    np.testing.assert_array_equal(d_pcol, pcol, err_msg=f"{what}: pcol")
    np.testing.assert_array_equal(d_pval.view(np.uint64), pval.view(np.uint64), err_msg=f"{what}: pval")


def csr_from_lengths(lens, K, seed, unsorted=False):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    p = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    rows = np.repeat(np.arange(lens.size), lens)
    j = rng.integers(0, K, size=int(p[-1])).astype(np.int32)
    if not unsorted:
        j = j[np.lexsort((j, rows))]
    k = rng.integers(1, 17, size=j.size) * rng.choice([-1, 1], size=j.size)
    return p.astype(np.int32), j, k.astype(np.float64) / 8.0


def mixed_lengths(m, seed):
    """m not a multiple of 64; empty rows, an empty octet, bundles of 256 < len <= 384 (staged, two passes of loads)
    and octets too long for the LDS stage (the scattered path)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 60, size=m)
    lens[rng.random(m) < 0.1] = 0
    lens[128:192] = 0                                   # octet 2 empty
    lens[64 * 5:64 * 6] = np.minimum(lens[64 * 5:64 * 6], 40)
    lens[64 * 5:64 * 5 + 8] = 48                        # a 384-step bundle: the largest staged octet
    lens[64 * 7 + 8:64 * 7 + 16] = 130                  # a 1040-entry bundle: scattered
    lens[-3:] = 0                                       # the last octet ends on empty rows
    return lens


def test_plan_model_holds_every_entry_once():
    """The restatement itself: each CSR entry in exactly one slot, everything else a no-op entry."""
    K = 300
    p, j, x = csr_from_lengths(mixed_lengths(64 * 9 + 3, seed=1), K, seed=2)
    for P in (1, 4, 64):
        step_off, pcol, pval, total = plan_model(p, j, x, K, P)
        col = pcol & ((1 << ROW_SHIFT) - 1)
        real = col < K
        assert real.sum() == j.size and np.all(pval[~real] == 0) and np.all(col[~real] == K)
        assert np.array_equal(np.sort(pval[real]), np.sort(x))
        assert total * 8 >= j.size and total % 32 == 0 and step_off[-1] == total
        assert np.all(np.diff(step_off) >= 0)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 3, 5, 8, 64])
def test_plan_bytes_match_layout(gpu, P):
    K = 4099
    p, j, x = csr_from_lengths(mixed_lengths(64 * 37 + 21, seed=P), K, seed=100 + P)
    A = DevCSR(p, j, x, K)
    plan = plan_create(A, npanels=P)
    try:
        assert_plan_equal(plan, p, j, x, K, P, f"P={P}")
    finally:
        _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [5, 64])
def test_plan_bytes_unsorted_rows(gpu, P):
    K = 70_001
    p, j, x = csr_from_lengths(mixed_lengths(3001, seed=7), K, seed=8, unsorted=True)
    A = DevCSR(p, j, x, K)
    plan = plan_create(A, npanels=P)
    try:
        assert_plan_equal(plan, p, j, x, K, P, f"unsorted P={P}")
    finally:
        _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
def test_plan_bytes_lognormal_rows(gpu):
    K = 100_000
    rng = np.random.default_rng(3)
    for sigma in (0.5, 1.3):
        lens = np.maximum(0, np.round(rng.lognormal(np.log(20), sigma, size=50_000))).astype(np.int64)
        p, j, x = csr_from_lengths(lens, K, seed=int(sigma * 10))
        A = DevCSR(p, j, x, K)
        plan = plan_create(A, npanels=0)
        try:
            assert_plan_equal(plan, p, j, x, K, None, f"log-normal sigma={sigma}")
        finally:
            _lib.load().mxd_spmm_plan_destroy(plan)


@pytest.mark.gpu
def test_plan_rebuilt_in_place_grows_and_shrinks(gpu):
    """A plan object re-used for a larger matrix has to grow its buffers and fill again; then a smaller one again."""
    K = 9000
    small = csr_from_lengths(mixed_lengths(200, seed=1), K, seed=2)
    big = csr_from_lengths(mixed_lengths(64 * 300 + 5, seed=3), K, seed=4)
    plan = None
    try:
        for step, (p, j, x) in enumerate((small, big, small, big)):
            A = DevCSR(p, j, x, K)
            plan = plan_create(A, npanels=6, plan=plan)
            assert_plan_equal(plan, p, j, x, K, 6, f"step {step} (m={p.size - 1})")
    finally:
        if plan is not None:
            _lib.load().mxd_spmm_plan_destroy(plan)


def _auto_expect(p):
    """AUTO's pad rule restated: reject when the plan holds more than 1.75 x nnz + 65536 slots."""
    m = p.size - 1
    noct = -(-m // 64)
    bl = np.diff(p.astype(np.int64)[np.minimum(np.arange(noct * 8 + 1) * 8, m)])
    total = int(((bl.reshape(noct, 8).max(axis=1) + 31) // 32 * 32).sum())
    return ROWWAVE if 32 * total > 7 * int(p[-1]) + 262144 else PLANNED


@pytest.mark.gpu
def test_auto_lognormal_rows_both_sides_of_the_pad_rule(gpu):
    """Log-normal row lengths under and over AUTO's 1.75x rule: the kernel AUTO runs follows the rule and C is exact
    (integer data, see exact_B in test_gpu_spmm_variants)."""
    lib = _lib.load()
    lib.mxd_release_workspaces()                                     # AUTO's first call has to grow its buffers
    K, n, m = 70_001, 16, (1 << 20) + 37
    rng = np.random.default_rng(11)
    for sigma, expect in ((0.5, PLANNED), (1.3, ROWWAVE)):
        lens = np.maximum(0, np.round(rng.lognormal(np.log(8), sigma, size=m))).astype(np.int64)
        p, j, x = csr_from_lengths(lens, K, seed=int(sigma * 10))
        assert _auto_expect(p) == expect, sigma
        k = (x * 8).astype(np.int64)
        L = np.random.default_rng(5).integers(-16, 17, size=(K, n)).astype(np.int64)
        B = L.astype(np.float64) / 16
        ref = (sp.csr_matrix((k, j, p), shape=(m, K)) @ L) / 128.0
        A = DevCSR(p, j, x, K)
        for colmajor in (True, False):
            got, err = spmm_guarded(A, B, colmajor, algo=0, rows_sorted=True)
            assert err is None, err
            assert last_kernel() == expect, (sigma, last_kernel())
            np.testing.assert_array_equal(got, ref, err_msg=f"AUTO sigma={sigma} colmajor={colmajor}")
