"""Every SpMM kernel variant against references that do not depend on summation order.

mxd_spmm_csr_dense_ex has three kernels (row-wave, slab, planned), each instantiated for dtype, output layout and
operand alignment; the planned kernel also for 16 / 8 / 4 waves per workgroup.  The tests here drive each of them
with B and C placed inside guarded device buffers (devmem.Guarded: element offset 0 or 1, leading dimension exact,
+VEC or +1, sentinel guard bands) and check:

  * exact data: A's values are k/8 and B's entries l/16 with small integers k, l, so every partial sum is exact in
    f64 and in f32 (the f32 path narrows each a to float).  Every kernel must equal the integer product bit for bit,
    whatever order it sums in;
  * NaN poison: rows of B that no entry of A references, and B's padding columns, are NaN; a NaN in C means a
    stray read went into an FMA;
  * guards: the guard bands, the offset and the ldc padding of C are bit-identical to the sentinel afterwards;
  * one random-normal case per kernel against an np.longdouble reference with the a-priori bound
    |C - C_ref| <= (len_row + 2) u (|A||B|);
  * which kernel ran (mxd_spmm_last_kernel), and that slab / planned refuse operands that break their 16-byte
    rules without touching C, while AUTO falls back to the row-wave kernel.

The large-column cases need a few GB of device memory (the slab-major copy of B is K x 128 B: 2.6 GB for the planned
case, 4.3 GB for the K >= 2^25 one); the export cases move more than 16 MiB each way through the pinned-slot copy
engine and are checked against the CPU oracle.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from devmem import DevCSR, last_kernel, plan_create, spmm_guarded
from matrixextra_amd import _lib
from matrixextra_amd import exports as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROWWAVE, SLAB, PLANNED = "spmm_rowwave_kernel", "spmm_slab_kernel", "spmm_plan_kernel"
ALGO_AUTO, ALGO_ROWWAVE, ALGO_SLAB, ALGO_PLANNED = 0, 1, 2, 3
DTYPES = [np.float64, np.float32]
DT_IDS = ["f64", "f32"]


def vec(dtype):
    return 16 // np.dtype(dtype).itemsize            # elements per 16-byte access


def slab_ns(dtype):
    v, w = vec(dtype), 128 // np.dtype(dtype).itemsize   # slab width W = one 128-byte line
    return [v, w - v, w, w + v, 3 * w + v]


def rowwave_ns(dtype):
    return slab_ns(dtype) + [1, 7, 64 * vec(dtype) + vec(dtype)]    # odd n, n = 1, one wavefront-wide pass + VEC


# (b_offset, ldb - n, c_offset, ldc - exact ldc); "V" = VEC
LAYOUTS = {
    "exact": (0, 0, 0, 0),
    "ld+vec": (0, "V", 0, "V"),
    "ld+1": (0, 1, 0, 1),
    "b_off": (1, 0, 0, 0),
    "c_ld+1": (0, 0, 0, 1),
    "c_off": (0, 0, 1, 0),
    "all_off": (1, 1, 1, 1),
}


def layout_args(name, dtype, m, n, colmajor):
    v = vec(dtype)
    bo, bx, co, cx = (v if a == "V" else a for a in LAYOUTS[name])
    return dict(b_offset=bo, ldb=n + bx, c_offset=co, ldc=(m if colmajor else n) + cx)


def qualifies(dtype, n, colmajor, b_offset, ldb, c_offset, ldc):
    """The slab / planned kernels' 16-byte rules (slab_ok in spmm_common.h), restated."""
    v, isz = vec(dtype), np.dtype(dtype).itemsize
    if n < v or n % v or ldb % v or (b_offset * isz) % 16:
        return False
    return colmajor or (ldc % v == 0 and (c_offset * isz) % 16 == 0)


# ------------------------------------------------------------------------------------------------ exact data
def exact_csr(m, K, seed, unsorted=False, long_rows=True):
    """Rows of 0..11 entries (row 0 empty, a few rows of 65..150), columns drawn with replacement from a random half
    of [1, K) (duplicates inside a row, column 0 never used), values k/8 with k in [-16, 16] \\ {0}.
    Returns (indptr, indices, values, integer values k)."""
    rng = np.random.default_rng(seed)
    used = rng.choice(np.arange(1, K), size=max(1, (K - 1) // 2), replace=False)
    lens = rng.integers(0, 12, size=m)
    if long_rows:
        lens[rng.random(m) < 0.01] = rng.integers(65, 151)
        lens[m // 2] = 97
    lens[0] = 0
    p = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    j = rng.choice(used, size=int(p[-1])).astype(np.int32)
    if not unsorted:
        rows = np.repeat(np.arange(m), lens)
        j = j[np.lexsort((j, rows))]
    k = rng.integers(1, 17, size=j.size) * rng.choice([-1, 1], size=j.size)
    return p.astype(np.int32), j, k / 8.0, k


def exact_B(p, j, K, n, dtype, seed):
    """B = l/16 with l in [-16, 16] on the rows A references, NaN on every other row.  Returns (B, integer l)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(-16, 17, size=(K, n), dtype=np.int8)
    ref_rows = np.zeros(K, dtype=bool)
    ref_rows[j] = True
    L[~ref_rows] = 0
    B = L.astype(dtype)
    B /= 16
    B[~ref_rows] = np.nan
    return B, L


def exact_ref(p, j, k, L, dtype):
    m, K = p.size - 1, L.shape[0]
    Ci = sp.csr_matrix((k.astype(np.int64), j, p), shape=(m, K)) @ L          # integer product (duplicates summed)
    return (np.asarray(Ci) / 128.0).astype(dtype)


class Case:
    """One exact-data matrix on the device with its B generator and integer reference."""

    def __init__(self, m, K, seed, unsorted=False, long_rows=True):
        self.m, self.K = m, K
        self.p, self.j, self.x, self.k = exact_csr(m, K, seed, unsorted, long_rows)
        self.A = DevCSR(self.p, self.j, self.x, K)
        self.seed = seed

    def B(self, n, dtype):
        B, L = exact_B(self.p, self.j, self.K, n, dtype, self.seed * 1000 + n)
        return B, exact_ref(self.p, self.j, self.k, L, dtype)


def check_exact(got, ref, what):
    assert got is not None, what
    assert not np.isnan(got).any(), f"{what}: NaN in C (a poisoned row or padding column of B reached an FMA)"
    np.testing.assert_array_equal(got, ref, err_msg=what)


_CASES = {}


def case(m, K=700, seed=None, unsorted=False):
    key = (m, K, seed, unsorted)
    if key not in _CASES:
        _CASES[key] = Case(m, K, seed if seed is not None else m + 3 * K, unsorted)
    return _CASES[key]


# m: < 64, a multiple of 8 but not of 64, and one that is a multiple of none of 8 / 64 / 256 / 512 / 1024
M_SMALL = [37, 1283]
M_PLANNED = [37, 1000, 1283]


# ------------------------------------------------------------------------------------------------ row-wave
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rowwave_variants(gpu, dtype, colmajor, layout):
    for m in M_SMALL:
        c = case(m)
        for n in rowwave_ns(dtype):
            B, ref = c.B(n, dtype)
            got, err = spmm_guarded(c.A, B, colmajor, algo=ALGO_ROWWAVE, **layout_args(layout, dtype, m, n, colmajor))
            assert err is None, err
            assert last_kernel() == ROWWAVE
            check_exact(got, ref, f"row-wave m={m} n={n}")


def test_rowwave_unsorted_rows(gpu):
    c = case(1283, unsorted=True)
    for dtype in DTYPES:
        for colmajor in (False, True):
            B, ref = c.B(3 * 128 // np.dtype(dtype).itemsize + vec(dtype), dtype)
            got, err = spmm_guarded(c.A, B, colmajor, algo=ALGO_ROWWAVE)
            assert err is None, err
            check_exact(got, ref, "row-wave, unsorted rows")


# ------------------------------------------------------------------------------------------------ slab
SLAB_KNOBS = {
    "wg1": (1, {}), "wg2": (2, {}), "wg4": (4, {}),
    "unpacked_wg1": (1, {"MXGPU_SLAB_PACK": "0"}),
    "rpg16_wg2": (2, {"MXGPU_SLAB_RPG": "16"}),
    "unpacked_rpg16_wg4": (4, {"MXGPU_SLAB_PACK": "0", "MXGPU_SLAB_RPG": "16"}),
}


@pytest.mark.parametrize("knobs", list(SLAB_KNOBS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_slab_variants(gpu, monkeypatch, dtype, colmajor, layout, knobs):
    wg, env = SLAB_KNOBS[knobs]
    for key, val in env.items():
        monkeypatch.setenv(key, val)                  # read by the library on every call
    for m in M_SMALL:
        c = case(m)
        for n in slab_ns(dtype):
            la = layout_args(layout, dtype, m, n, colmajor)
            ok = qualifies(dtype, n, colmajor, **la)
            B, ref = c.B(n, dtype)
            for npanels in (1, 3):
                got, err = spmm_guarded(c.A, B, colmajor, algo=ALGO_SLAB, rows_sorted=True, npanels=npanels,
                                        wg_per_cu=wg, **la)
                what = f"slab m={m} n={n} npanels={npanels}"
                if not ok:
                    assert err is not None and "16-byte alignment rules" in err, (what, err)
                    continue
                assert err is None, (what, err)
                assert last_kernel() == SLAB
                check_exact(got, ref, what)


def test_slab_unsorted_rows(gpu, monkeypatch):
    c = case(1283, unsorted=True)
    for pack in ("1", "0"):
        monkeypatch.setenv("MXGPU_SLAB_PACK", pack)
        for dtype in DTYPES:
            for colmajor in (False, True):
                B, ref = c.B(3 * 128 // np.dtype(dtype).itemsize + vec(dtype), dtype)
                got, err = spmm_guarded(c.A, B, colmajor, algo=ALGO_SLAB, rows_sorted=False, npanels=4)
                assert err is None, err
                assert last_kernel() == SLAB
                check_exact(got, ref, "slab, unsorted rows (panels forced to 1)")


# ------------------------------------------------------------------------------------------------ planned
def _planned_panels(m):
    return {37: 1, 1000: 5}.get(m, 3)


@pytest.mark.parametrize("wg", [1, 2, 4], ids=["wg1", "wg2", "wg4"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_planned_plan_api_variants(gpu, dtype, colmajor, layout, wg):
    lib = _lib.load()
    for m in M_PLANNED:
        c = case(m)
        plan = plan_create(c.A, npanels=_planned_panels(m))
        try:
            for n in slab_ns(dtype):
                la = layout_args(layout, dtype, m, n, colmajor)
                ok = qualifies(dtype, n, colmajor, **la)
                B, ref = c.B(n, dtype)
                for sync in (0, 1, 2):
                    got, err = spmm_guarded(c.A, B, colmajor, plan=plan, wg_per_cu=wg, sync_mode=sync, **la)
                    what = f"planned m={m} n={n} sync={sync}"
                    if not ok:
                        assert err is not None and "16-byte alignment rules" in err, (what, err)
                        continue
                    assert err is None, (what, err)
                    assert last_kernel() == PLANNED
                    check_exact(got, ref, what)
        finally:
            lib.mxd_spmm_plan_destroy(plan)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_planned_ex_variants(gpu, dtype, colmajor, layout):
    for m in M_SMALL:
        c = case(m)
        for n in slab_ns(dtype):
            la = layout_args(layout, dtype, m, n, colmajor)
            ok = qualifies(dtype, n, colmajor, **la)
            B, ref = c.B(n, dtype)
            got, err = spmm_guarded(c.A, B, colmajor, algo=ALGO_PLANNED, npanels=_planned_panels(m), **la)
            what = f"planned (_ex) m={m} n={n}"
            if not ok:
                assert err is not None and "16-byte alignment rules" in err, (what, err)
                continue
            assert err is None, (what, err)
            assert last_kernel() == PLANNED
            check_exact(got, ref, what)


def test_planned_unsorted_rows(gpu):
    c = case(1283, unsorted=True)
    lib = _lib.load()
    plan = plan_create(c.A, npanels=4)
    try:
        for dtype in DTYPES:
            for colmajor in (False, True):
                B, ref = c.B(3 * 128 // np.dtype(dtype).itemsize + vec(dtype), dtype)
                for wg in (1, 2, 4):
                    got, err = spmm_guarded(c.A, B, colmajor, plan=plan, wg_per_cu=wg, sync_mode=1)
                    assert err is None, err
                    check_exact(got, ref, f"planned, unsorted rows, wg_per_cu={wg}")
    finally:
        lib.mxd_spmm_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ AUTO (small)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_auto_small_variants(gpu, dtype, colmajor, layout):
    for m in M_SMALL:
        c = case(m)
        for n in rowwave_ns(dtype):
            B, ref = c.B(n, dtype)
            got, err = spmm_guarded(c.A, B, colmajor, algo=ALGO_AUTO, rows_sorted=True,
                                    **layout_args(layout, dtype, m, n, colmajor))
            assert err is None, err
            assert last_kernel() == ROWWAVE                 # B fits one XCD's L2: AUTO stays on the row-wave kernel
            check_exact(got, ref, f"AUTO m={m} n={n}")


# ------------------------------------------------------------------------------------------------ rounding bound
def _bounded_run(kernel, A, B, colmajor, monkeypatch):
    if kernel == "rowwave":
        return spmm_guarded(A, B, colmajor, algo=ALGO_ROWWAVE), ROWWAVE
    if kernel == "slab":
        return spmm_guarded(A, B, colmajor, algo=ALGO_SLAB, rows_sorted=True, npanels=3), SLAB
    if kernel == "slab_unpacked":
        monkeypatch.setenv("MXGPU_SLAB_PACK", "0")
        return spmm_guarded(A, B, colmajor, algo=ALGO_SLAB, rows_sorted=True, npanels=3, wg_per_cu=2), SLAB
    if kernel == "planned_ex":
        return spmm_guarded(A, B, colmajor, algo=ALGO_PLANNED, npanels=3), PLANNED
    if kernel == "auto":
        return spmm_guarded(A, B, colmajor, algo=ALGO_AUTO, rows_sorted=True), ROWWAVE
    lib = _lib.load()
    plan = plan_create(A, npanels=5)
    try:
        return spmm_guarded(A, B, colmajor, plan=plan, wg_per_cu=int(kernel[-1]), sync_mode=2), PLANNED
    finally:
        lib.mxd_spmm_plan_destroy(plan)


@pytest.mark.parametrize("kernel", ["rowwave", "slab", "slab_unpacked", "planned_ex", "plan_wg1", "plan_wg2",
                                    "plan_wg4", "auto"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_random_normal_within_rounding_bound(gpu, monkeypatch, dtype, kernel):
    m, K = 1283, 2000
    n = 3 * 128 // np.dtype(dtype).itemsize + vec(dtype)
    p, j, _, _ = exact_csr(m, K, seed=5)
    rng = np.random.default_rng(6)
    x = rng.normal(size=j.size)
    B = rng.normal(size=(K, n)).astype(dtype)
    A = DevCSR(p, j, x, K)
    colmajor = kernel in ("slab", "plan_wg2", "auto")
    (got, err), expect_kernel = _bounded_run(kernel, A, B, colmajor, monkeypatch)
    assert err is None, err
    assert last_kernel() == expect_kernel
    # reference on the values the kernel multiplies (a narrowed to float on the f32 path), in long double
    a = x.astype(dtype).astype(np.longdouble)
    Bl = B.astype(np.longdouble)
    rows = np.repeat(np.arange(m), np.diff(p))
    ref = np.zeros((m, n), dtype=np.longdouble)
    np.add.at(ref, rows, a[:, None] * Bl[j])
    mag = np.zeros((m, n))
    np.add.at(mag, rows, np.abs(x.astype(dtype).astype(np.float64))[:, None] * np.abs(B.astype(np.float64))[j])
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    bound = (np.diff(p)[:, None] + 2) * u * mag
    err_abs = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    assert np.isfinite(got).all()
    worst = np.argmax(err_abs - bound)
    assert (err_abs <= bound).all(), f"{kernel}: |C - ref| = {err_abs.flat[worst]:.3e} > {bound.flat[worst]:.3e}"


# ------------------------------------------------------------------------------------------------ plan lifecycle
def test_one_plan_many_runs(gpu):
    """One plan against several B, widths, dtypes and layouts, interleaved."""
    lib = _lib.load()
    c = case(1283, K=2000)
    plan = plan_create(c.A, npanels=6)
    try:
        for rep in range(2):
            for dtype in DTYPES:
                v, w = vec(dtype), 128 // np.dtype(dtype).itemsize
                for n, colmajor, layout in ((v, False, "exact"), (3 * w, True, "c_off"), (w + v, False, "ld+vec"),
                                            (v, True, "c_ld+1")):
                    n += rep * v
                    B, ref = c.B(n, dtype)
                    got, err = spmm_guarded(c.A, B, colmajor, plan=plan, **layout_args(layout, dtype, c.m, n, colmajor))
                    assert err is None, err
                    check_exact(got, ref, f"plan run rep={rep} n={n} {layout}")
    finally:
        lib.mxd_spmm_plan_destroy(plan)


def test_plan_object_reused_across_matrices(gpu):
    """*plan_out non-null: the plan of a larger matrix is rebuilt in place for a smaller one and back."""
    lib = _lib.load()
    big, small = case(5000, K=4000), case(37, K=50)
    plan = plan_create(big.A, npanels=7)
    try:
        for step, (c, npanels) in enumerate(((big, 7), (small, 2), (big, 3), (small, 0), (big, 7))):
            if step:
                assert plan_create(c.A, npanels=npanels, plan=plan).value == plan.value
            for dtype, colmajor in ((np.float64, True), (np.float32, False)):
                B, ref = c.B(128 // np.dtype(dtype).itemsize + vec(dtype), dtype)
                got, err = spmm_guarded(c.A, B, colmajor, plan=plan)
                assert err is None, err
                check_exact(got, ref, f"reused plan, step {step} (m={c.m})")
    finally:
        lib.mxd_spmm_plan_destroy(plan)


def test_plan_create_refuses_2_pow_25_columns(gpu):
    lib = _lib.load()
    A = DevCSR(np.array([0, 1], dtype=np.int32), np.array([5], dtype=np.int32), np.array([1.0]), 1 << 25)
    plan = C.c_void_p()
    rc = lib.mxd_spmm_plan_create(C.c_int(1), C.c_int(1 << 25), A.dp.ptr, A.dj.ptr, A.dx.ptr, C.c_int(0), None,
                                  C.byref(plan))
    assert rc != 0 and plan.value is None
    assert "more than 2^25 columns" in lib.mx_last_error().decode()


def _uniform_csr(m, K, per_row, seed):
    rng = np.random.default_rng(seed)
    used = rng.choice(np.arange(1, K), size=K // 2, replace=False)
    j = np.sort(rng.choice(used, size=(m, per_row)), axis=1).reshape(-1).astype(np.int32)
    p = (np.arange(m + 1, dtype=np.int64) * per_row).astype(np.int32)
    k = rng.integers(1, 17, size=j.size) * rng.choice([-1, 1], size=j.size)
    return p, j, k


def _one_bundle_per_octet_csr(m, K, seed):
    """Rows 0..7 of every 64-row octet hold 32 entries, the other 56 rows one: the plan would be ~6.6x the CSR."""
    rng = np.random.default_rng(seed)
    lens = np.where(np.arange(m) % 64 < 8, 32, 1)
    p = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    rows = np.repeat(np.arange(m), lens)
    j = rng.integers(1, K, size=int(p[-1])).astype(np.int32)
    j = j[np.lexsort((j, rows))]
    k = rng.integers(1, 17, size=j.size) * rng.choice([-1, 1], size=j.size)
    return p.astype(np.int32), j, k


def test_auto_plan_and_workspaces_across_matrices(gpu):
    """AUTO keeps its plan and the packed B in grow-only thread-local buffers; run it across matrices of different
    shape, one of them rejected as over-padded, and across mxd_release_workspaces().  Every step is exact."""
    lib = _lib.load()
    K, n = 70_001, 16                           # B = 9 MB f64 (> one XCD's L2), m * n >= 2^24: AUTO's planned range
    m = (1 << 20) + 37

    def run(p, j, k, Kc, expect, **layout):
        A = DevCSR(p, j, k / 8.0, Kc)
        B, L = exact_B(p, j, Kc, n, np.float64, seed=int(p.size))
        ref = exact_ref(p, j, k, L, np.float64)
        for colmajor in (True, False):
            got, err = spmm_guarded(A, B, colmajor, algo=ALGO_AUTO, rows_sorted=True, **layout)
            assert err is None, err
            assert last_kernel() == expect, (expect, last_kernel())
            check_exact(got, ref, f"AUTO m={A.m} expect {expect} {layout}")

    uni = _uniform_csr(m, K, 8, seed=1)
    run(*uni, K, PLANNED)                                            # 1. uniform rows: planned
    run(*_one_bundle_per_octet_csr(m, K, seed=2), K, ROWWAVE)        # 2. over-padded plan rejected: row-wave
    run(*uni, K, ROWWAVE, b_offset=1)                                #    B 8 bytes off: row-wave
    small = case(1283, K=K)
    run(small.p, small.j, small.k, K, ROWWAVE)                       # 3. small: row-wave
    run(*uni, K, PLANNED)                                            # 4. first matrix again
    assert lib.mxd_release_workspaces() == 0
    run(*uni, K, PLANNED)                                            # 5. after the workspaces were freed


# ------------------------------------------------------------------------------------------------ large columns
def _checksum(got, p, j, k, L):
    """1^T C == (A^T 1)^T B, in integers (C = integer product / 128)."""
    w = np.bincount(j, weights=k, minlength=L.shape[0]).astype(np.int64)
    np.testing.assert_array_equal(got.astype(np.float64).sum(axis=0) * 128.0, (w @ L).astype(np.float64))


def _csr_on_columns(m, cols, per_row, seed):
    rng = np.random.default_rng(seed)
    j = np.sort(rng.choice(np.asarray(cols), size=(m, per_row)), axis=1).reshape(-1).astype(np.int32)
    p = (np.arange(m + 1, dtype=np.int64) * per_row).astype(np.int32)
    k = rng.integers(1, 17, size=j.size) * rng.choice([-1, 1], size=j.size)
    return p, j, k


def test_planned_columns_above_2_pow_24(gpu):
    """Planned kernel, f32, n = 4, K ~ 20M: entries at and around panel boundaries above 2^24, where panel_of's float
    estimate is no longer exact and the correction step decides.  ~3 GB of device memory (packed B: K x 128 B)."""
    lib = _lib.load()
    K, n, m = 20_000_003, 4, 3001
    special = {K - 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1}
    for npanels in (64, 7):
        pc = -(-K // npanels)
        for b in range(pc, K, pc):
            if b >= (1 << 24) - 1:
                special |= {b - 1, b, b + 1}
    rng = np.random.default_rng(3)
    cols = np.array(sorted(c for c in special if c < K) + list(rng.integers(1 << 24, K, size=200)))
    p, j, k = _csr_on_columns(m, cols, 12, seed=4)
    A = DevCSR(p, j, k / 8.0, K)
    B, L = exact_B(p, j, K, n, np.float32, seed=5)
    ref = exact_ref(p, j, k, L, np.float32)
    for npanels in (0, 64, 7):                     # 0: default (64 at this K)
        plan = plan_create(A, npanels=npanels)
        try:
            got, err = spmm_guarded(A, B, npanels == 7, plan=plan, wg_per_cu=2 if npanels else 1)
            assert err is None, err
            assert last_kernel() == PLANNED
            check_exact(got, ref, f"planned K={K} npanels={npanels}")
            _checksum(got, p, j, k, L)
        finally:
            lib.mxd_spmm_plan_destroy(plan)


def test_auto_selects_slab_at_2_pow_25_columns(gpu):
    """AUTO with K >= 2^25 (the planned kernel's limit) runs the slab kernel; exact on every row plus the column
    checksum.  ~5 GB of device memory."""
    lib = _lib.load()
    K, n, m = (1 << 25) + 3, 4, (1 << 22) + 5    # f32 B = 537 MB, m * n >= 2^24
    rng = np.random.default_rng(7)
    cols = np.concatenate([[1, K - 1, K - 2, (1 << 25) - 1, 1 << 25, (1 << 24) + 1],
                           rng.integers(1, K, size=4096)])
    p, j, k = _csr_on_columns(m, cols, 2, seed=8)
    A = DevCSR(p, j, k / 8.0, K)
    B, L = exact_B(p, j, K, n, np.float32, seed=9)
    ref = exact_ref(p, j, k, L, np.float32)
    try:
        got, err = spmm_guarded(A, B, True, algo=ALGO_AUTO, rows_sorted=True)
        assert err is None, err
        assert last_kernel() == SLAB
        check_exact(got, ref, f"AUTO K={K}")
        _checksum(got, p, j, k, L)
    finally:
        lib.mxd_release_workspaces()


# ------------------------------------------------------------------------------------------------ export transfers
def _assert_lists_equal(g, o):
    for key in ("indptr", "indices", "values"):
        assert g[key].dtype == o[key].dtype and g[key].shape == o[key].shape, key
        np.testing.assert_array_equal(g[key], o[key], err_msg=key)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_tcrossprod_export_large_transfers(gpu, dtype):
    """Y > 16 MiB and A's values > 16 MiB in, a result of >= 4 chunks of 8 MiB back whose byte count is a multiple
    of neither 8 MiB nor 4 KiB (odd element count): every transfer runs through the pipelined pinned-slot engine."""
    m, K, n = 700_001, 400_003, 13
    p, j, k = _uniform_csr(m, K, 4, seed=11)
    x = k / 8.0
    rng = np.random.default_rng(12)
    Y = np.asfortranarray((rng.integers(-16, 17, size=(n, K)) / 16.0).astype(dtype))
    assert Y.nbytes > 16 << 20 and x.nbytes > 16 << 20
    assert m * n % 2 == 1 and m * n * np.dtype(dtype).itemsize > 4 * (8 << 20)
    fn = G.tcrossprod_csr_dense_numeric if dtype == np.float64 else G.tcrossprod_csr_dense_float32
    got = fn(p, j, x, Y, 1)
    ref = O.tcrossprod_csr_dense(p, j, x, Y, 1, use_fma=True)
    assert got.shape == (m, n) and got.dtype == dtype and got.flags.f_contiguous
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, exact_ref(p, j, k, (Y.T * 16).astype(np.int8), dtype))


def test_elemwise_and_row_gather_exports_large_results(gpu):
    from matrixextra_amd import synth
    m, K = 600_001, 1_000_000
    p, j, x = synth.csr_fixed(m, K, 8, seed=21)
    p2, j2, x2 = synth.csr_overlapping(p, j, K, 8, seed=22)
    g, o = G.add_csr_elemwise(p, p2, j, j2, x, x2, False), O.add_csr_elemwise(p, p2, j, j2, x, x2, False)
    assert g["values"].nbytes > 16 << 20 and g["indices"].nbytes > 16 << 20
    _assert_lists_equal(g, o)
    rows = synth.rows_with_replacement(600_001, m)
    g, o = G.copy_csr_rows_numeric(p, j, x, rows), O.copy_csr_rows_numeric(p, j, x, rows)
    assert g["values"].nbytes > 16 << 20 and g["indices"].nbytes > 16 << 20
    _assert_lists_equal(g, o)


def test_device_layer_column_view_of_B(gpu):
    """device.spmm passes B.stride(0) as ldb, so a column view such as Bwide[:, 1:] reaches the kernels with ldb > n
    and B 8 bytes off a 16-byte boundary: AUTO / row-wave run it, the planned kernel refuses it."""
    import torch
    from matrixextra_amd import device as D
    c = case(1283)
    Bw, ref = c.B(17, np.float64)
    ref = ref[:, 1:]
    A = D.DeviceCSR.from_host(c.p, c.j, c.x, c.K)
    view = torch.from_numpy(Bw).cuda()[:, 1:]
    assert view.stride(0) == 17 and view.data_ptr() % 16 == 8
    for colmajor in (False, True):
        check_exact(D.spmm(A, view, colmajor=colmajor).cpu().numpy(), ref, f"device.spmm colmajor={colmajor}")
        assert last_kernel() == ROWWAVE
        with pytest.raises(_lib.MxError, match="16-byte alignment rules"):
            D.spmm_planned(A, view, colmajor=colmajor)
