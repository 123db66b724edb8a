"""The device-level entry points of include/mxgpu_dense.h against the numpy model of tests/dense_model.py, bit for bit:
indptr and indices as int32, values as their bits.  Every operand and every output lies between guard bytes (the
device memory of tests/devmem.py); outputs start as 0xFF bytes, so an element never written, or written past the end,
shows; the padding rows of a dense operand hold a non-zero poison that must not come back, those of a dense output
must still hold 0xFF.

Shapes: every (m, n) with m, n in {1, 63, 64, 65, 129} (below, at and above the 64-row panel and the 64-column chunk,
and two of each), 0 x 5, 5 x 0, and 200 x 3 / 3 x 200 (four panels of one short chunk; one panel of four chunks).  Each
shape runs with by_col 1 and with by_col 0 at col_splits 0, 1, 2, 3, at ld = m and ld = m + 3, at densities 0, 5 %,
50 % and 1, and the twelve (input kind, output kind) pairs go round over those runs; test_every_kind_pair crosses them
in full at one shape."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dense_model as DM
import devmem
import streams as ST
from dense_model import NA, NA_REAL, bits
from matrixextra_amd import _lib
from streams import B, Case, H, In, IO, Out, Row, Step, Ws

SIZES = (1, 63, 64, 65, 129)
SHAPES = list(itertools.product(SIZES, SIZES)) + [(0, 5), (5, 0), (200, 3), (3, 200)]
CONFIGS = [(1, 0)] + [(0, s) for s in (0, 1, 2, 3)]                    # (by_col, col_splits)
DENSITIES = (0.0, 0.05, 0.5, 1.0)
KINDS = {"f64": (np.float64, _lib.MX_F64), "f32": (np.float32, _lib.MX_F32), "i32": (np.int32, _lib.MX_I32),
         "lgl": (np.int32, _lib.MX_LGL)}
OUTS = {"d": (np.float64, _lib.MX_F64), "l": (np.int32, _lib.MX_LGL), "n": (None, _lib.MX_NONE)}
PAIRS = list(itertools.product(KINDS, OUTS))
OTHER_NAN = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]     # a NaN with a payload of its own
GUARD = devmem.GUARD_BYTES


def lib():
    return _lib.load()


class Buf:
    """n elements of `dtype` in device memory between guards: `data`, or 0xFF bytes for an output."""

    def __init__(self, dtype, n=None, data=None):
        self.dtype = np.dtype(dtype)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=self.dtype).reshape(-1)
            n = data.size
        self.n = int(n)
        self.nbytes = -(-self.n * self.dtype.itemsize // 16) * 16
        host = np.tile(devmem.GUARD_PATTERN, (2 * GUARD + self.nbytes) // 4)
        host[GUARD:GUARD + self.nbytes] = 0xFF
        if data is not None:
            host[GUARD:GUARD + data.nbytes] = data.view(np.uint8)
        self.expect = host
        self.dev = devmem.Dev(host)
        self.ptr = C.c_void_p(self.dev.ptr.value + GUARD)

    def payload(self):
        """the bytes between the guards, after asserting that the guards are what was uploaded"""
        got = self.dev.download(np.uint8, self.expect.shape)
        for name, sl in (("front", slice(0, GUARD)), ("back", slice(GUARD + self.nbytes, None))):
            bad = np.flatnonzero(got[sl] != self.expect[sl])
            assert bad.size == 0, f"{bad.size} byte(s) of the {name} guard changed, first at byte {int(bad[0])} of it"
        return got[GUARD:GUARD + self.nbytes]

    def result(self, written=None):
        """the first `written` elements (default all): none of them still 0xFF bytes, everything behind them is"""
        written = self.n if written is None else int(written)
        body = self.payload()
        isz = self.dtype.itemsize
        untouched = (body.reshape(-1, isz) == 0xFF).all(axis=1)
        left = np.flatnonzero(untouched[:written])
        assert left.size == 0, f"{left.size} of {written} element(s) never written, first at {int(left[0])}"
        stray = np.flatnonzero(~untouched[written:])
        assert stray.size == 0, f"{stray.size} element(s) written past the end {written}, first at {written + int(stray[0])}"
        return body[:written * isz].view(self.dtype).copy()

    def assert_untouched(self):
        got = self.dev.download(np.uint8, self.expect.shape)
        bad = np.flatnonzero(got != self.expect)
        assert bad.size == 0, f"{bad.size} byte(s) of an input changed, first at byte {int(bad[0]) - GUARD}"


def sync():
    _lib.check(lib().mx_stream_sync(None))


def make_dense(m, n, kind, density, seed):
    """an m x n matrix of `kind` with about `density` cells kept, the special cells of the kind among them, an empty
    first row, an empty last row and a full row in the middle (at the two middle densities, where there is room)"""
    rng = np.random.default_rng(seed)
    dtype = KINDS[kind][0]
    keep = rng.random((m, n)) < density
    if kind in ("f64", "f32"):
        D = np.where(keep, np.round(rng.normal(size=(m, n)), 2) + 3.0, 0.0).astype(dtype)
        special = [-0.0, np.inf, -np.inf, OTHER_NAN if kind == "f64" else np.float32(np.nan), NA_REAL if kind == "f64" else 1.5]
    elif kind == "i32":
        D = np.where(keep, rng.integers(1, 100, size=(m, n)), 0).astype(dtype)
        special = [NA, -7, 2**31 - 1]
    else:
        D = np.where(keep, 1, 0).astype(dtype)
        special = [NA]
    free = np.ones(m, dtype=bool)                                       # rows the special cells may fall into
    if 0.0 < density < 1.0 and m >= 3:
        D[0, :] = 0
        D[m - 1, :] = 0
        D[m // 2, :] = 1
        free[[0, m // 2, m - 1]] = False
    cells = np.flatnonzero(np.repeat(free, n))
    if density > 0.0 and cells.size:
        at = rng.choice(cells, size=min(cells.size, 2 * len(special)), replace=False)
        D.reshape(-1)[at] = np.resize(np.array(special, dtype=dtype), at.size)
    return D


def padded(D, ld, poison):
    """the column-major image of D at leading dimension ld, `poison` in the padding rows"""
    m, n = D.shape
    img = np.full((n, ld), poison, dtype=D.dtype)
    img[:, :m] = D.T
    return img.reshape(-1)


def dev_dense_to_csr(D, kind, ld, by_col, col_splits, out):
    """mxd_dense_to_csr_count + _fill on guarded buffers: (indptr, indices, values or None)"""
    m, n = D.shape
    nseg = n if by_col else m
    gd = Buf(D.dtype, data=padded(D, ld, 77))
    gws = Buf(np.uint8, n=lib().mxd_dense_to_csr_workspace_bytes(m, n, by_col, col_splits))
    gp, total = Buf(np.int32, n=nseg + 1), C.c_int64(-1)
    _lib.check(lib().mxd_dense_to_csr_count(m, n, gd.ptr, ld, KINDS[kind][1], by_col, col_splits, gp.ptr, gws.ptr,
                                            C.byref(total), None))
    nnz = int(total.value)
    vdt, code = OUTS[out]
    gj = Buf(np.int32, n=nnz + devmem.SLACK)
    gx = None if vdt is None else Buf(vdt, n=nnz + devmem.SLACK)
    _lib.check(lib().mxd_dense_to_csr_fill(m, n, gd.ptr, ld, KINDS[kind][1], by_col, col_splits, gp.ptr, gws.ptr, gj.ptr,
                                           None if gx is None else gx.ptr, code, None))
    sync()
    gd.assert_untouched()
    gws.payload()
    indptr = gp.result()
    assert indptr[-1] == nnz
    return indptr, gj.result(nnz), None if gx is None else gx.result(nnz)


def dev_csr_to_dense(p, j, x, nother, ld, by_col, col_splits, logical, expect_flag=0):
    """mxd_csr_to_dense into a guarded, 0xFF-filled matrix at leading dimension ld: the m x n block (None when the
    flag is expected: the content is then unspecified), after asserting the flag, the guards and the padding rows"""
    nseg = p.size - 1
    m, n = (nother, nseg) if by_col else (nseg, nother)
    gp, gj = Buf(np.int32, data=p), Buf(np.int32, data=j)
    gx = None if x is None else Buf(x.dtype, data=x)
    odt = np.int32 if logical else np.float64
    gout, gflag = Buf(odt, n=ld * n), Buf(np.int32, data=np.zeros(1, np.int32))
    vd = _lib.MX_NONE if x is None else _lib.MX_F64 if x.dtype == np.float64 else _lib.MX_LGL
    _lib.check(lib().mxd_csr_to_dense(nseg, nother, gp.ptr, gj.ptr, None if gx is None else gx.ptr, vd, by_col, col_splits,
                                      gout.ptr, ld, _lib.MX_LGL if logical else _lib.MX_F64, gflag.ptr, None))
    sync()
    for g in (gp, gj, gx):
        if g is not None:
            g.assert_untouched()
    assert gflag.payload()[:4].view(np.int32)[0] == expect_flag
    isz = np.dtype(odt).itemsize
    raw = gout.payload()[:ld * n * isz].reshape(n, ld, isz)
    assert (raw[:, m:] == 0xFF).all(), "a padding row of the output was written"
    if expect_flag:
        return None
    assert not (raw[:, :m] == 0xFF).all(axis=2).any(), "a cell of the output was never written"
    block = np.ascontiguousarray(raw[:, :m]).view(odt).reshape(n, m)
    return np.asfortranarray(block.T)


def same(got, want, what):
    assert (got is None) == (want is None), what
    if want is not None:
        assert got.dtype == want.dtype and got.shape == want.shape, what
        assert np.array_equal(bits(got), bits(want)), what


def run_both_ways(D, kind, ld, by_col, col_splits, out, logical):
    """dense -> compressed against the model, then its arrays back to a dense matrix against the model"""
    what = f"{D.shape} {kind}->{out} ld {ld} by_col {by_col} col_splits {col_splits}"
    p, j, x = DM.dense_to_csr(D, kind, by_col, out)
    got = dev_dense_to_csr(D, kind, ld, by_col, col_splits, out)
    for g, w, name in zip(got, (p, j, x), ("indptr", "indices", "values")):
        same(g, w, f"{what}: {name}")
    nother = D.shape[0] if by_col else D.shape[1]
    back = dev_csr_to_dense(p, j, x, nother, ld, by_col, col_splits, logical)
    same(back, DM.csr_to_dense(p, j, x, nother, by_col, logical), f"{what}: back to dense, logical {logical}")
    if kind == "f64" and out == "d" and not logical:                   # the kept cells' bits, +0.0 elsewhere
        same(back, np.asfortranarray(np.where(D != 0, D, 0.0)), f"{what}: round trip")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_shape(gpu, m, n):
    run = 0
    for (by_col, col_splits), pad, density in itertools.product(CONFIGS, (0, 3), DENSITIES):
        kind, out = PAIRS[(run + m + 5 * n) % len(PAIRS)]
        D = make_dense(m, n, kind, density, seed=[m, n, run])
        run_both_ways(D, kind, m + pad, by_col, col_splits, out, logical=run % 2 == 1)
        run += 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind,out", PAIRS, ids=[f"{k}-{o}" for k, o in PAIRS])
def test_every_kind_pair(gpu, kind, out):
    D = make_dense(65, 129, kind, 0.5, seed=[7, len(kind), ord(out)])
    assert (D[0] == 0).all() and (D[-1] == 0).all() and (D[32] != 0).all()
    if kind == "f64":
        assert np.isin(bits(np.array([OTHER_NAN, NA_REAL, np.inf, -np.inf])), bits(D)).all() and (bits(D) == 1 << 63).any()
    elif kind != "f32":
        assert (D == NA).any()
    for (by_col, col_splits), logical in itertools.product(((1, 0), (0, 0), (0, 3)), (False, True)):
        first = run_both_ways(D, kind, 68, by_col, col_splits, out, logical)
        again = dev_dense_to_csr(D, kind, 68, by_col, col_splits, out)         # the same bits on every call
        for a, b in zip(first, again):
            same(a, b, "second call")


def test_the_model_keeps_what_the_issue_says():
    D = np.array([[0.0, -0.0, np.nan], [np.inf, 2.0, NA_REAL]])
    p, j, x = DM.dense_to_csr(D, "f64", False, "d")
    assert p.tolist() == [0, 1, 4] and j.tolist() == [2, 0, 1, 2] and bits(x)[3] == 0x7FF00000000007A2
    assert DM.dense_to_csr(D, "f64", False, "l")[2].tolist() == [NA, 1, 1, NA]
    Di = np.array([[NA, 0], [5, 1]], np.int32)
    assert bits(DM.dense_to_csr(Di, "i32", True, "d")[2]).tolist() == [0x7FF00000000007A2, bits(np.array([5.0]))[0],
                                                                       bits(np.array([1.0]))[0]]
    assert DM.dense_to_csr(Di, "lgl", False, "l")[2].tolist() == [NA, 5, 1]      # a logical is copied


# ---- arrays that are no matrix ---------------------------------------------------------------------------------------
BAD = {   # 3 segments, indices below 70: (indptr, indices)
    "repeated": ([0, 3, 3, 4], [1, 5, 5, 2]),
    "unsorted": ([0, 3, 3, 4], [1, 66, 5, 2]),
    "too_large": ([0, 3, 3, 4], [1, 5, 70, 2]),
    "negative": ([0, 3, 3, 4], [-1, 5, 6, 2]),
    "last_of_the_row_large": ([0, 2, 2, 4], [1, 5, 2, 2**31 - 1]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(BAD))
@pytest.mark.parametrize("by_col,col_splits", CONFIGS)
def test_offending_entries_set_the_flag_and_write_nothing_outside(gpu, case, by_col, col_splits):
    p, j = (np.array(a, np.int32) for a in BAD[case])
    for x, logical in ((np.arange(1.0, 5.0), False), (None, True)):
        m = 70 if by_col else 3
        assert dev_csr_to_dense(p, j, x, 70, m + 3, by_col, col_splits, logical, expect_flag=1) is None


@pytest.mark.gpu
def test_long_segments_cross_the_row_ranges_of_a_column(gpu):
    """by_col = 1 gives a wave 4096 rows of a column: 9000 rows are three ranges, found by binary search"""
    rng = np.random.default_rng(5)
    D = np.where(rng.random((9000, 3)) < 0.3, rng.normal(size=(9000, 3)), 0.0)
    D[4095:4097, 1] = 1.0
    D[:, 2] = 0.0
    p, j, x = DM.dense_to_csr(D, "f64", True, "d")
    same(dev_csr_to_dense(p, j, x, 9000, 9001, 1, 0, False), np.asfortranarray(D), "three ranges")
    j[p[1] - 1] = 8999                                                  # fine: still ascending
    j[p[1] + 5] = j[p[1] + 4]                                           # a repeat inside the second column
    assert dev_csr_to_dense(p, j, x, 9000, 9000, 1, 0, False, expect_flag=1) is None


# ---- a side stream behind pending work -------------------------------------------------------------------------------
def stream_row():
    m, n, splits = 129, 200, 2

    def make(v):
        D = make_dense(m, n, "f64", 0.3, seed=[11, v])
        p, j, x = DM.dense_to_csr(D, "f64", False, "d")
        bufs = dict(D=In(np.asfortranarray(D).reshape(-1, order="F")), out_p=Out(np.int32, p), out_j=Out(np.int32, j),
                    out_x=Out(np.float64, x), ws=Ws(lib().mxd_dense_to_csr_workspace_bytes(m, n, 0, splits)),
                    Ap=In(p), Aj=In(j), Ax=In(x), flag=IO(np.zeros(1, np.int32), np.zeros(1, np.int32)),
                    dense=Out(np.float64, DM.csr_to_dense(p, j, x, n, False, False).reshape(-1, order="F")))
        return Case(bufs, [
            Step("mxd_dense_to_csr_count", [m, n, B("D"), m, _lib.MX_F64, 0, splits, B("out_p"), B("ws"), H("nnz")],
                 late=("D",), waits=True, host=dict(nnz=int(p[-1]))),
            Step("mxd_dense_to_csr_fill", [m, n, B("D"), m, _lib.MX_F64, 0, splits, B("out_p"), B("ws"), B("out_j"),
                                           B("out_x"), _lib.MX_F64], late=("D",)),
            Step("mxd_csr_to_dense", [m, n, B("Ap"), B("Aj"), B("Ax"), _lib.MX_F64, 0, splits, B("dense"), m, _lib.MX_F64,
                                      B("flag")], late=("Ap", "Aj", "Ax"))])
    return Row("dense_rows_two_splits", make)


STREAM_ROW = stream_row()
STREAM_STEPS = list(range(3))


@pytest.mark.gpu
@pytest.mark.parametrize("k", STREAM_STEPS, ids=STREAM_ROW.entry_points())
def test_ordered_on_a_side_stream(gpu, k):
    ST.run_ordered(STREAM_ROW, k)
