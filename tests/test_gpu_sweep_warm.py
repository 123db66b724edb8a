"""The warm hand-over of the planned sweep (spmm_plan_kernel, column-major): a wavefront whose tile of
C is full requests the first 8 B lines of its next work item in front of its stores of C and enters that item through a
copy of the chunk body that starts at k = 1.  Every other hand-over is cold: no octet, a partial tile (rows or columns),
no next item, a next item with an empty stream, or a held plan chunk that is not the next item's first one.

Which hand-overs a shape meets is derived on the CPU from the kernel's item map and the plan's step_off (the numpy
restatement of the plan in test_gpu_plan_build.py), and every case asserts the counts it is there for before it runs.
Checked as in test_gpu_sweep_carry.py, whose matrices, references and tolerances these tests share: the output buffer
starts as NaN, every case runs twice into the same buffer and the second result must equal the first bit for bit; f64
rtol 1e-12, atol 1e-11 and f32 rtol = atol = 1e-5 against the non-FMA oracle, compared on the device.
"""
import collections
import functools

import numpy as np
import pytest

from matrixextra_amd import synth
from oracle import oracle as O
from test_gpu_plan_build import plan_model
from test_gpu_sweep_carry import GEN_ROWS, K, M, _assert_close, _matrix, _operands

pytestmark = pytest.mark.gpu

# 160 generations less 24 rows (the last octet is partial).  With n = 24 / 40 (two slabs, the second one partial) that
# is 320 items, 40 per XCD group over 32 workgroups: workgroups 0..7 of a group have a second item.  With n = 132
# (nine slabs) it is 1440 items, 180 per group: five or six items per workgroup, 32 generations apart, so most
# hand-overs stay inside a slab, and group 7 crosses from slab 7 into the partial slab 8.
M_LONG = 160 * GEN_ROWS - 24


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _step_off(kind, m, P):
    p, j, x = _matrix(kind, m)
    return plan_model(p, j, x, K, P)[0].astype(np.int64)


def handovers(so, P, m, n, W, cus, wg_per_cu=1):
    """Counter of the kinds of hand-over the column-major sweep meets, per wavefront: the kernel's item map (see
    test_gpu_sweep_carry.handover_kinds), its grid (wg_per_cu workgroups of 16 / wg_per_cu wavefronts per CU, at most
    items + 7, a multiple of 8), the step each read-ahead leaves in the held chunk, and the kernel's warm rule, restated."""
    WAVES = 16 // wg_per_cu
    noct, ngens, nslabs = -(-m // 64), -(-m // (64 * WAVES)), -(-n // W)
    total = nslabs * ngens
    nwg = max(min(cus * wg_per_cu, total + 7) // 8 * 8, 8) // 8
    kinds = collections.Counter()
    for xcd in range(8):
        lo, hi = total * xcd // 8, total * (xcd + 1) // 8
        niter = -(-(hi - lo) // nwg)
        for wg in range(nwg):
            items = list(range(lo + wg, hi, nwg))
            for w in range(WAVES):
                held = -1
                for it in range(niter):
                    have = it < len(items)
                    slab, gen = divmod(items[it], ngens) if have else (0, 0)
                    oct = gen * WAVES + w
                    oct_ok = have and oct < noct
                    sbeg, send = (so[oct * P], so[oct * P + P]) if oct_ok else (0, 0)
                    nslab, ngen = divmod(items[it + 1], ngens) if it + 1 < len(items) else (0, 0)
                    noct_next = ngen * WAVES + w
                    n_ok = it + 1 < len(items) and noct_next < noct
                    n_beg, n_end = (so[noct_next * P], so[noct_next * P + P]) if n_ok else (-2, -2)
                    if send > sbeg:                              # the stream's last read-ahead
                        held = n_beg if n_ok else send
                    if not have:
                        continue
                    if not oct_ok:
                        kinds["cold: no octet"] += 1
                    elif oct * 64 + 64 > m:
                        kinds["cold: partial rows"] += 1
                    elif n - slab * W < W:
                        kinds["cold: partial slab"] += 1
                    elif not n_ok:
                        kinds["cold: no next item"] += 1
                    elif n_end <= n_beg:
                        kinds["cold: next stream empty"] += 1
                    elif held != n_beg:
                        kinds["cold: held chunk is not the next item's first"] += 1
                    else:
                        kinds["warm, same slab" if nslab == slab else "warm, other slab"] += 1
                        if n - nslab * W < W:
                            kinds["warm into the partial slab"] += 1
                        if P > 1 and so[noct_next * P + 1] == n_beg:
                            kinds["warm, panel 0 of the next octet is empty"] += 1
    return kinds


@functools.lru_cache(maxsize=None)
def _long_operands(n, dtype):
    """Fixed rows, M_LONG x K, few columns of B: host CSR, device CSR, device B, the oracle's product on the device."""
    import torch
    from matrixextra_amd import device as D
    p, j, x = synth.csr_fixed(M_LONG, K, 12, seed=M_LONG + K)
    B = synth.dense_normal(K, n, dtype=dtype)
    ref = O.tcrossprod_csr_dense(p, j, x, np.asfortranarray(B.T), 1).astype(np.float64)
    return (p, j, x), D.DeviceCSR.from_host(p, j, x, K), torch.from_numpy(B).cuda(), torch.from_numpy(ref).cuda()


def _run_twice(A, dB, m, n, dtype, colmajor, npanels, sync_mode, wg_per_cu=0):
    import torch
    from matrixextra_amd import device as D
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out = torch.full((n, m) if colmajor else (m, n), float("nan"), dtype=tdt, device="cuda")
    D.spmm_planned(A, dB, out=out, colmajor=colmajor, npanels=npanels, wg_per_cu=wg_per_cu, sync_mode=sync_mode)
    first = out.clone()
    D.spmm_planned(A, dB, out=out, colmajor=colmajor, npanels=npanels, wg_per_cu=wg_per_cu, sync_mode=sync_mode)
    assert torch.equal(first.view(torch.uint8), out.view(torch.uint8)), \
        "second call into the same buffer differs from the first"
    return first.t() if colmajor else first


def _check(ops, m, n, dtype, colmajor, npanels, sync_mode, wg_per_cu=0):
    _, A, dB, ref = ops
    got = _run_twice(A, dB, m, n, dtype, colmajor, npanels, sync_mode, wg_per_cu)
    assert tuple(got.shape) == tuple(ref.shape)
    _assert_close(got, ref, dtype)


@pytest.mark.parametrize("sync_mode", [0, 1, 2])
@pytest.mark.parametrize("npanels", [1, 8, 64])
def test_lognormal_warm_across_slabs(gpu, npanels, sync_mode):
    """64 slabs x 13 generations: a workgroup's next item is 32 items on, in another slab (other base of B) and six
    generations on, behind a stream of another length.  At 64 panels of 24 columns, panel 0 of some octets is empty:
    the meeting at that boundary falls on the skipped k = 0 and is caught up by k = 1."""
    kinds = handovers(_step_off("lognormal", M, npanels), npanels, M, 1024, 16, _cus())
    assert kinds["warm, other slab"] > 0 and kinds["cold: no next item"] > 0 and kinds["cold: partial rows"] > 0, kinds
    if npanels == 64:
        assert kinds["warm, panel 0 of the next octet is empty"] > 0, kinds
    _check(_operands("lognormal", M, 1024, np.float64), M, 1024, np.float64, True, npanels, sync_mode)


@pytest.mark.parametrize("wg_per_cu", [1, 2, 4])
def test_workgroups_per_cu(gpu, wg_per_cu):
    """One workgroup of 16 wavefronts per CU, two of 8, four of 4: each has its own kernel, item map and grid.  Lognormal
    rows, the matrix with emptied generations and octets, and f32."""
    kinds = handovers(_step_off("lognormal", M, 8), 8, M, 1024, 16, _cus(), wg_per_cu)
    assert kinds["warm, same slab"] + kinds["warm, other slab"] > 0 and kinds["cold: no next item"] > 0 and \
        kinds["cold: partial rows"] > 0, kinds
    _check(_operands("lognormal", M, 1024, np.float64), M, 1024, np.float64, True, 8, 1, wg_per_cu)
    kinds = handovers(_step_off("holes", M, 8), 8, M, 1024, 16, _cus(), wg_per_cu)
    assert kinds["cold: next stream empty"] > 0 and kinds["cold: held chunk is not the next item's first"] > 0 and \
        kinds["warm, same slab"] + kinds["warm, other slab"] > 0, kinds
    _check(_operands("holes", M, 1024, np.float64), M, 1024, np.float64, True, 8, 1, wg_per_cu)
    _check(_operands("lognormal64", M, 2048, np.float32), M, 2048, np.float32, True, 8, 1, wg_per_cu)


@pytest.mark.parametrize("npanels", [1, 8])
def test_holes_cold_behind_and_in_front_of_empty_streams(gpu, npanels):
    """test_gpu_sweep_carry's matrix with whole generations and single octets emptied: a next item with an empty stream
    is entered cold, and so is the item behind it (its first chunk was never read ahead); around them the hand-overs
    are warm, and wavefronts of one workgroup differ."""
    kinds = handovers(_step_off("holes", M, npanels), npanels, M, 1024, 16, _cus())
    assert kinds["cold: next stream empty"] > 0 and kinds["cold: held chunk is not the next item's first"] > 0 and \
        kinds["warm, other slab"] > 0 and kinds["cold: no octet"] > 0, kinds
    for sync_mode in (0, 1, 2) if npanels > 1 else (0,):
        _check(_operands("holes", M, 1024, np.float64), M, 1024, np.float64, True, npanels, sync_mode)


@pytest.mark.parametrize("extra", [1, 65])
def test_one_or_two_octets_in_the_last_generation(gpu, extra):
    """m = 1024 g + 1 and + 65: the last generation has one partial octet, or a full one and a partial one; the other
    wavefronts have no octet there and none to hand over to."""
    m = 12 * GEN_ROWS + extra
    kinds = handovers(_step_off("fixed", m, 8), 8, m, 1024, 16, _cus())
    assert kinds["cold: partial rows"] > 0 and kinds["cold: no octet"] > 0 and kinds["cold: no next item"] > 0 and \
        kinds["warm, other slab"] > 0, kinds
    _check(_operands("fixed", m, 1024, np.float64), m, 1024, np.float64, True, 8, 1)
    _check(_operands("lognormal", m, 1024, np.float64), m, 1024, np.float64, True, 8, 1)


@pytest.mark.parametrize("n,dtype", [(24, np.float64), (132, np.float64), (40, np.float32)])
def test_partial_last_slab(gpu, n, dtype):
    """A last slab of 8 (f64: n = 24), 4 (n = 132) or 8 (f32: n = 40) columns: its tiles go out through the guarded
    epilogue and hand over cold; with nine slabs a hand-over from a full slab into the partial one is warm, and most
    warm hand-overs stay inside a slab (same base of B)."""
    W = 16 if dtype == np.float64 else 32
    ops = _long_operands(n, dtype)
    p, j, x = ops[0]
    so = plan_model(p, j, x, K, 8)[0].astype(np.int64)
    kinds = handovers(so, 8, M_LONG, n, W, _cus())
    assert kinds["cold: partial slab"] > 0 and kinds["cold: partial rows"] > 0 and kinds["cold: no next item"] > 0, kinds
    assert kinds["warm, same slab"] + kinds["warm, other slab"] > 0, kinds
    if n == 132:
        assert kinds["warm, same slab"] > 0 and kinds["warm, other slab"] > 0 and \
            kinds["warm into the partial slab"] > 0, kinds
    _check(ops, M_LONG, n, dtype, True, 8, 1)


def test_float32_column_major(gpu):
    """32 stores per tile in front of the warm entry; rows cut at 64 entries (see test_gpu_sweep_carry)."""
    kinds = handovers(_step_off("lognormal64", M, 8), 8, M, 2048, 32, _cus())
    assert kinds["warm, other slab"] > 0, kinds
    _check(_operands("lognormal64", M, 2048, np.float32), M, 2048, np.float32, True, 8, 1)
    _check(_operands("lognormal64", M, 2048, np.float32), M, 2048, np.float32, True, 8, 2)


def test_row_major_untouched(gpu):
    _check(_operands("lognormal", M, 1024, np.float64), M, 1024, np.float64, False, 8, 1)


def test_bit_identical_to_one_item_per_workgroup(gpu):
    """As in test_gpu_sweep_carry: the rows of the big call (warm hand-overs) again as calls on blocks of 4096 rows,
    64 slabs x 4 generations = 256 items, one per workgroup and nothing handed over.  The bytes must be the same."""
    import torch
    from matrixextra_amd import device as D
    P, n, block = 8, 1024, GEN_ROWS * 32 // 8
    (p, j, x), A, dB, _ = _operands("lognormal", M, n, np.float64)
    assert handovers(_step_off("lognormal", M, P), P, M, n, 16, _cus())["warm, other slab"] > 0
    big = _run_twice(A, dB, M, n, np.float64, True, P, 1)
    for b0 in range(0, M, block):
        b1 = min(b0 + block, M)
        pb, jb, xb = (p[b0:b1 + 1] - p[b0]).astype(np.int32), j[p[b0]:p[b1]], x[p[b0]:p[b1]]
        Ab = D.DeviceCSR.from_host(pb, jb, xb, K)
        assert -(-n // 16) * -(-(b1 - b0) // GEN_ROWS) <= 256
        part = D.spmm_planned(Ab, dB, colmajor=True, npanels=P, wg_per_cu=0, sync_mode=1)
        assert torch.equal(part.contiguous().view(torch.uint8), big[b0:b1].contiguous().view(torch.uint8)), \
            f"rows {b0}..{b1} differ from the one-item-per-workgroup call"
