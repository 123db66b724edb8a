"""The planned sweep's prefetch chain (spmm_plan_kernel): the octet's panel boundaries held in a register and
everything that is carried from one generation of a workgroup to the next.  Shapes are chosen for what that chain can
get wrong: work items that do not exist, empty octets, bundles that end early, every panel count / workgroup shape /
meeting mode, partial slabs.  Every case runs twice into the same output buffer and the second result must have the
same bytes as the first (a stale prefetched chunk or a missed re-zeroing of the accumulators shows up there).

Tolerances are those of the existing planned-kernel tests: f64 rtol 1e-12 (atol 1e-11, as in
test_spmm_planned_kernel_skewed_unsorted_special) against the non-FMA oracle, f32 rtol = atol = 1e-5."""
import functools

import numpy as np
import pytest

from matrixextra_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _with_empty_rows(p, j, x, empty):
    """The CSR (p, j, x) with the rows in `empty` (boolean mask) emptied."""
    lens = np.diff(p).astype(np.int64)
    keep = np.repeat(~empty, lens)
    lens[empty] = 0
    q = np.zeros(p.size, dtype=np.int32)
    np.cumsum(lens, out=q[1:])
    return q, j[keep], x[keep]


@functools.lru_cache(maxsize=None)
def _matrix(kind, m, K, per_row):
    if kind == "fixed":
        return synth.csr_fixed(m, K, per_row, seed=m + K)
    if kind == "lognormal":                                  # boundaries differ per bundle, some bundles end early
        return synth.csr_skewed(m, K, per_row, seed=m + K)
    assert kind == "holes"
    p, j, x = synth.csr_fixed(m, K, per_row, seed=m + K)
    empty = np.zeros(m, dtype=bool)
    empty[:64] = True                                        # the first octet
    empty[m - (m % 64 or 64) - 64:] = True                   # the last two octets (the last one may be partial)
    empty[1024:2048] = True                                  # a whole generation of a 16-wave workgroup
    empty[2048 + 128:2048 + 320] = True                      # whole octets inside a generation
    empty[2600:2610] = True                                  # and a few rows inside an octet
    return _with_empty_rows(p, j, x, empty)


@functools.lru_cache(maxsize=None)
def _operands(kind, m, K, per_row, n, dtype):
    p, j, x = _matrix(kind, m, K, per_row)
    B = synth.dense_normal(K, n, dtype=dtype)
    ref = O.tcrossprod_csr_dense(p, j, x, np.asfortranarray(B.T), 1).astype(np.float64)     # non-FMA oracle
    return p, j, x, B, ref


def _check(kind, m, K, per_row, n, dtype, colmajor, npanels, wg_per_cu, sync_mode):
    import torch
    from matrixextra_amd import device as D
    p, j, x, B, ref = _operands(kind, m, K, per_row, n, dtype)
    A = D.DeviceCSR.from_host(p, j, x, K)
    dB = torch.from_numpy(B).cuda()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out = torch.full((n, m) if colmajor else (m, n), float("nan"), dtype=tdt, device="cuda")
    got = []
    for _ in range(2):
        res = D.spmm_planned(A, dB, out=out, colmajor=colmajor, npanels=npanels, wg_per_cu=wg_per_cu,
                             sync_mode=sync_mode)
        torch.cuda.synchronize()
        got.append(res.cpu().numpy().copy())
    assert got[0].shape == ref.shape
    if dtype == np.float64:
        np.testing.assert_allclose(got[0], ref, rtol=1e-12, atol=1e-11)
    else:
        np.testing.assert_allclose(got[0].astype(np.float64), ref, rtol=1e-5, atol=1e-5)
    assert got[0].tobytes() == got[1].tobytes(), "second call into the same buffer differs from the first"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("colmajor", [True, False])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1023, 1025])
def test_row_counts_around_octet_and_generation_edges(gpu, m, colmajor, dtype):
    """fewer work items than workgroups: most workgroups have no item at all, the last octet is partial"""
    _check("fixed", m, 300, 5, 128, dtype, colmajor, 2, 0, -1)


@pytest.mark.parametrize("dtype,colmajor", [(np.float64, True), (np.float32, False)])
@pytest.mark.parametrize("wg_per_cu", [1, 2, 4])
def test_idle_workgroups_in_last_iteration(gpu, wg_per_cu, dtype, colmajor):
    """m = 40000, n = 128 f64: 8 slabs x 40 / 79 / 157 generations over 32 / 64 / 128 workgroups per XCD group, so
    the last iteration runs with most workgroups idle (the item after a workgroup's last one does not exist)"""
    _check("fixed", 40000, 2000, 6, 128, dtype, colmajor, 8, wg_per_cu, -1)


@pytest.mark.parametrize("sync_mode", [0, 1, 2])
@pytest.mark.parametrize("npanels", [1, 2, 8, 64])
def test_empty_octets_first_last_and_whole_generations(gpu, npanels, sync_mode):
    for dtype, colmajor in ((np.float64, True), (np.float32, False)):
        _check("holes", 3000, 1500, 12, 64, dtype, colmajor, npanels, 0, sync_mode)


@pytest.mark.parametrize("sync_mode", [0, 1, 2])
@pytest.mark.parametrize("wg_per_cu", [1, 2, 4])
@pytest.mark.parametrize("npanels", [1, 2, 8, 64])
def test_lognormal_rows_every_shape_of_the_sweep(gpu, npanels, wg_per_cu, sync_mode):
    _check("lognormal", 5000, 2500, 24, 128, np.float64, True, npanels, wg_per_cu, sync_mode)


@pytest.mark.parametrize("colmajor", [True, False])
@pytest.mark.parametrize("wg_per_cu", [1, 2, 4])
def test_lognormal_rows_float32_and_rowmajor(gpu, wg_per_cu, colmajor):
    _check("lognormal", 5000, 2500, 24, 128, np.float32, colmajor, 8, wg_per_cu, 1)
    _check("lognormal", 5000, 2500, 24, 128, np.float64, colmajor, 8, wg_per_cu, 2)


@pytest.mark.parametrize("colmajor", [True, False])
@pytest.mark.parametrize("dtype,n", [(np.float64, 24), (np.float64, 132), (np.float32, 40), (np.float32, 132)])
def test_partial_last_slab(gpu, dtype, n, colmajor):
    """n is not a multiple of the slab width (16 f64 / 32 f32 columns)"""
    _check("lognormal", 5000, 2500, 24, n, dtype, colmajor, 8, 0, -1)
    _check("holes", 3000, 1500, 12, n, dtype, colmajor, 2, 2, -1)
