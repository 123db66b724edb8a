"""What the planned sweep (spmm_plan_kernel) carries from one work item of a workgroup to its next one: the next
octet's bounds and its first plan chunk.  Only a workgroup's second and later items ever use a carried value, so the
shapes here have many slabs and few generations: m ~ 13 000 rows (13 generations of 1024 rows), n = 1024 f64 / 2048 f32
columns (64 slabs) give 832 items, 104 per XCD group over 32 workgroups of 16 wavefronts: three or four items each,
the last round only partly filled.

Checked as in test_gpu_sweep_pipeline.py: the output buffer starts as NaN, every case runs twice into the same buffer
and the second result must equal the first bit for bit; f64 rtol 1e-12, atol 1e-11 and f32 rtol = atol = 1e-5 against
the non-FMA oracle (that file's tolerances).  The comparisons run on the device (|got - ref| <= atol + rtol |ref|, which
a NaN fails), so that a case costs two launches and no 100 MB copy.
"""
import functools

import numpy as np
import pytest

from matrixextra_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

M, K = 13000, 1500                       # 13 generations of a 16-wave workgroup, the last one with 12 octets (one partial)
WAVES, GEN_ROWS = 16, 1024
EMPTY_GENS = (1, 4)                      # see test_holes: chosen so that every kind of hand-over occurs


def _with_empty_rows(p, j, x, empty):
    lens = np.diff(p).astype(np.int64)
    keep = np.repeat(~empty, lens)
    lens[empty] = 0
    q = np.zeros(p.size, dtype=np.int32)
    np.cumsum(lens, out=q[1:])
    return q, j[keep], x[keep]


@functools.lru_cache(maxsize=None)
def _matrix(kind, m):
    if kind == "fixed":
        return synth.csr_fixed(m, K, 12, seed=m + K)
    if kind == "lognormal":              # streams of different lengths from item to item, bundles that end early
        return synth.csr_skewed(m, K, 24, seed=m + K)
    if kind == "lognormal64":            # the same, rows cut at 64 entries: see test_lognormal_float32
        return synth.csr_skewed(m, K, 24, seed=m + K, max_nnz=64)
    assert kind == "holes"
    p, j, x = synth.csr_fixed(m, K, 12, seed=m + K)
    empty = np.zeros(m, dtype=bool)
    for g in EMPTY_GENS:                 # whole generations
        empty[g * GEN_ROWS:(g + 1) * GEN_ROWS] = True
    for g, octs in ((0, (0,)), (6, (3, 9)), (7, (15,)), (10, (0, 1, 2))):      # single octets inside a generation
        for o in octs:
            empty[g * GEN_ROWS + o * 64:g * GEN_ROWS + (o + 1) * 64] = True
    empty[m - (m % 64 or 64):] = True    # the last (partial) octet
    empty[2600:2610] = True              # and a few rows inside an octet
    return _with_empty_rows(p, j, x, empty)


@functools.lru_cache(maxsize=None)
def _operands(kind, m, n, dtype):
    """Host CSR, device CSR (keeps its plan), device B and the oracle's product on the device, made once."""
    import torch
    from matrixextra_amd import device as D
    p, j, x = _matrix(kind, m)
    B = synth.dense_normal(K, n, dtype=dtype)
    ref = O.tcrossprod_csr_dense(p, j, x, np.asfortranarray(B.T), 1).astype(np.float64)     # non-FMA oracle
    return (p, j, x), D.DeviceCSR.from_host(p, j, x, K), torch.from_numpy(B).cuda(), torch.from_numpy(ref).cuda()


def _assert_close(got, ref, dtype):
    import torch
    rtol, atol = (1e-12, 1e-11) if dtype == np.float64 else (1e-5, 1e-5)
    err = (got.to(torch.float64) - ref).abs()
    ok = err <= atol + rtol * ref.abs()                      # False for a NaN
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        raise AssertionError(f"{bad.shape[0]} of {ok.numel()} elements off (rtol {rtol}, atol {atol}); first at "
                             f"{tuple(bad[0].tolist())}: got {got[tuple(bad[0])].item()!r}, want {ref[tuple(bad[0])].item()!r}")


def _run_twice(A, dB, m, n, dtype, colmajor, npanels, sync_mode):
    import torch
    from matrixextra_amd import device as D
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out = torch.full((n, m) if colmajor else (m, n), float("nan"), dtype=tdt, device="cuda")
    D.spmm_planned(A, dB, out=out, colmajor=colmajor, npanels=npanels, wg_per_cu=0, sync_mode=sync_mode)
    first = out.clone()
    D.spmm_planned(A, dB, out=out, colmajor=colmajor, npanels=npanels, wg_per_cu=0, sync_mode=sync_mode)
    assert torch.equal(first.view(torch.uint8), out.view(torch.uint8)), \
        "second call into the same buffer differs from the first"
    return first.t() if colmajor else first


def _check(kind, m, n, dtype, colmajor, npanels, sync_mode):
    _, A, dB, ref = _operands(kind, m, n, dtype)
    got = _run_twice(A, dB, m, n, dtype, colmajor, npanels, sync_mode)
    assert tuple(got.shape) == tuple(ref.shape)
    _assert_close(got, ref, dtype)


@pytest.mark.parametrize("colmajor", [True, False])
@pytest.mark.parametrize("sync_mode", [0, 1, 2])
@pytest.mark.parametrize("npanels", [1, 8, 64])
def test_lognormal_three_items_per_workgroup(gpu, npanels, sync_mode, colmajor):
    _check("lognormal", M, 1024, np.float64, colmajor, npanels, sync_mode)


def test_lognormal_float32(gpu):
    """Rows cut at 64 entries, so that atol = 1e-5 bounds what a correct float32 sum may be off by.  A term a b (a
    uniform in [-1, 1], b standard normal) has rms 0.58, the partial sum after k terms 0.58 sqrt(k), and every addition
    rounds by up to 2^-24 of it: over a row of L entries the rounding adds up to about 2^-24 * 0.58 * L / sqrt(2) rms,
    1.6e-6 for L = 64 — six standard deviations below 1e-5, with 27 M elements checked.  The uncut log-normal rows
    reach several hundred entries (6e-6 rms for L = 250), and there a handful of the 27 M float32 elements lie
    1.0e-5 .. 1.5e-5 from the float64 oracle by rounding alone (measured: 5 elements, the worst 1.43e-5 off)."""
    _check("lognormal64", M, 2048, np.float32, True, 8, 1)
    _check("lognormal64", M, 2048, np.float32, False, 8, 2)


def handover_kinds(p, m, nslabs, grid=256, waves=WAVES):
    """The kinds of hand-over between consecutive work items that the sweep meets on (p, m) with `grid` workgroups of
    `waves` wavefronts.  The kernel's item map: XCD group x = workgroup % 8 owns items [total x / 8, total (x + 1) / 8),
    workgroup wg = workgroup / 8 of nwg = grid / 8 takes item = lo + wg + it nwg; generation = item % ngens, and
    wavefront w works on octet generation * waves + w.  Per wavefront an item is N (octet with entries), E (octet
    without) or X (no such octet)."""
    noct, ngens, nwg = -(-m // 64), -(-m // (64 * waves)), grid // 8
    total = nslabs * ngens
    p = np.asarray(p, dtype=np.int64)
    octs = np.arange(noct)
    filled = p[np.minimum((octs + 1) * 64, m)] > p[octs * 64]
    kinds = set()
    for xcd in range(8):
        lo, hi = total * xcd // 8, total * (xcd + 1) // 8
        niter = -(-(hi - lo) // nwg)
        for wg in range(nwg):
            gens = [item % ngens for item in range(lo + wg, hi, nwg)]
            if not gens:
                continue
            if len(gens) < niter:
                kinds.add("no next item: the last round is partly filled")
            per_wave = []
            for w in range(waves):
                st = "".join("X" if g * waves + w >= noct else "NE"[not filled[g * waves + w]] for g in gens)
                per_wave.append(st)
                if "NEN" in st:
                    kinds.add("non-empty > empty > non-empty")
                if st.startswith("EN"):
                    kinds.add("empty > non-empty as the first two items")
                if st.endswith("E"):
                    kinds.add("last item empty")
                if "NX" in st or "EX" in st:
                    kinds.add("next item without an octet")
            for it in range(len(gens) - 1):
                if len({st[it:it + 2] for st in per_wave}) > 1:
                    kinds.add("wavefronts of one workgroup hand over differently")
    return kinds, max(-(-(total * (x + 1) // 8 - total * x // 8) // nwg) for x in range(8))


def _skip_unless_256_cus():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the item map is derived for a grid of 256 workgroups, this device has {cus} CUs")


@pytest.mark.parametrize("colmajor", [True, False])
@pytest.mark.parametrize("npanels", [1, 8])
def test_holes_every_kind_of_handover(gpu, npanels, colmajor):
    """Fixed rows with generations 1 and 4 emptied, and single octets.  64 slabs x 13 generations = 8 slabs per XCD
    group, so workgroup wg starts at generation wg % 13 and moves on by 32 % 13 = 6: wg 8 sees 8, 1, 7 (non-empty,
    empty, non-empty), wg 1 sees 1, 7, 0 (empty first), wg 15 sees 2, 8, 1 (empty last); workgroups 8..31 have
    three items while 0..7 have four.  The kinds are derived from the kernel's item map, not from this reasoning."""
    _skip_unless_256_cus()
    p, _, _ = _matrix("holes", M)
    kinds, niter = handover_kinds(p, M, 64)
    assert niter >= 3
    assert kinds >= {"non-empty > empty > non-empty", "empty > non-empty as the first two items", "last item empty",
                     "no next item: the last round is partly filled", "next item without an octet",
                     "wavefronts of one workgroup hand over differently"}, kinds
    for sync_mode in (0, 1, 2) if npanels > 1 else (0,):
        _check("holes", M, 1024, np.float64, colmajor, npanels, sync_mode)
    if npanels == 8:
        _check("holes", M, 2048, np.float32, colmajor, npanels, 1)


@pytest.mark.parametrize("colmajor", [True, False])
@pytest.mark.parametrize("extra", [1, 65])
def test_one_or_two_octets_in_the_last_generation(gpu, extra, colmajor):
    """m just past a generation edge: the 13th generation has one (two) octets, so 15 (14) wavefronts of a workgroup
    carry "no next octet" into it while the others carry a real one."""
    m = 12 * GEN_ROWS + extra
    _check("fixed", m, 1024, np.float64, colmajor, 8, -1)
    _check("lognormal", m, 1024, np.float64, colmajor, 8, 1)


def test_bit_identical_to_one_item_per_workgroup(gpu):
    """The rows of the big call again as calls on blocks of 1024 * 32 / 8 = 4096 rows: 64 slabs x 4 generations = 256
    items, one per workgroup, so nothing is ever carried there.  Both must give the same bytes: a block starts on a
    bundle (8 rows) and octet boundary, and what a row adds up, in which order, is fixed by its bundle alone: the plan
    orders a bundle's entries by (panel, row, CSR position) with panels cut at col / panel_cols, the sweep adds them in
    that order.  That the block's plan is the same slots as the block's part of the big plan is checked first, on the
    host model of the plan (test_gpu_plan_build.plan_model)."""
    import torch
    from matrixextra_amd import device as D
    from test_gpu_plan_build import plan_model
    P, n, block = 8, 1024, GEN_ROWS * 32 // 8
    (p, j, x), A, dB, _ = _operands("lognormal", M, n, np.float64)
    so_big, pcol_big, pval_big, _ = plan_model(p, j, x, K, P)
    for colmajor in (True, False):
        big = _run_twice(A, dB, M, n, np.float64, colmajor, P, 1)
        for b0 in range(0, M, block):
            b1 = min(b0 + block, M)
            pb, jb, xb = (p[b0:b1 + 1] - p[b0]).astype(np.int32), j[p[b0]:p[b1]], x[p[b0]:p[b1]]
            if colmajor:
                so, pcol, pval, steps = plan_model(pb, jb, xb, K, P)
                s0 = int(so_big[b0 // 64 * P])
                assert np.array_equal(pcol[:steps * 8], pcol_big[s0 * 8:(s0 + steps) * 8])
                assert np.array_equal(pval[:steps * 8].view(np.uint64), pval_big[s0 * 8:(s0 + steps) * 8].view(np.uint64))
            Ab = D.DeviceCSR.from_host(pb, jb, xb, K)
            nitems = -(-n // 16) * -(-(b1 - b0) // GEN_ROWS)
            assert nitems <= 256
            part = D.spmm_planned(Ab, dB, colmajor=colmajor, npanels=P, wg_per_cu=0, sync_mode=1)
            assert torch.equal(part.contiguous().view(torch.uint8), big[b0:b1].contiguous().view(torch.uint8)), \
                f"rows {b0}..{b1} ({'column' if colmajor else 'row'}-major) differ from the one-item-per-workgroup call"
