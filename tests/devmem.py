"""Test helper: drive the device-level C-ABI (mxd_*) directly with library-managed device memory
(mx_dev_malloc / mx_memcpy_*), no torch involved."""
import ctypes as C

import numpy as np

from matrixextra_amd import _lib
from matrixextra_amd._lib import check


class Dev:
    """A numpy array mirrored into device memory for the lifetime of the object."""

    def __init__(self, arr=None, nbytes=None):
        lib = _lib.load()
        self.host = None if arr is None else np.ascontiguousarray(arr)
        self.nbytes = int(nbytes if arr is None else self.host.nbytes)
        self.ptr = C.c_void_p()
        check(lib.mx_dev_malloc(C.byref(self.ptr), max(self.nbytes, 16)))
        if self.host is not None and self.nbytes:
            check(lib.mx_memcpy_h2d(self.ptr, C.c_void_p(self.host.ctypes.data), self.nbytes, None))
            check(lib.mx_stream_sync(None))

    def download(self, dtype, shape):
        lib = _lib.load()
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            check(lib.mx_memcpy_d2h(C.c_void_p(out.ctypes.data), self.ptr, out.nbytes, None))
            check(lib.mx_stream_sync(None))
        return out

    def __del__(self):
        try:
            _lib.load().mx_dev_free(self.ptr)
        except Exception:
            pass


def spmm_device(p, j, x, B_rowmajor, colmajor, algo, rows_sorted, npanels=0, wg_per_cu=0):
    """C = A @ B through mxd_spmm_csr_dense_ex; returns C as an (m, n) numpy array."""
    lib = _lib.load()
    m, (K, n) = p.size - 1, B_rowmajor.shape
    dt = _lib.MX_F64 if B_rowmajor.dtype == np.float64 else _lib.MX_F32
    dp, dj, dx, dB = Dev(p.astype(np.int32)), Dev(j.astype(np.int32)), Dev(x.astype(np.float64)), Dev(B_rowmajor)
    dC = Dev(nbytes=m * n * B_rowmajor.dtype.itemsize)
    check(lib.mx_dev_memset(dC.ptr, 0xFF, dC.nbytes, None))      # poison: every element must be written
    check(lib.mxd_spmm_csr_dense_ex(m, n, K, dp.ptr, dj.ptr, dx.ptr, dB.ptr, n, dC.ptr, m if colmajor else n, dt,
                                    int(colmajor), algo, int(rows_sorted), npanels, wg_per_cu, None))
    check(lib.mx_stream_sync(None))
    out = dC.download(B_rowmajor.dtype, (n, m) if colmajor else (m, n))
    return out.T if colmajor else out


def spmm_planned_device(p, j, x, B_rowmajor, colmajor, npanels=0, wg_per_cu=0, sync_mode=-1):
    """C = A @ B through mxd_spmm_plan_create / mxd_spmm_plan_run; returns C as an (m, n) numpy array."""
    lib = _lib.load()
    m, (K, n) = p.size - 1, B_rowmajor.shape
    dt = _lib.MX_F64 if B_rowmajor.dtype == np.float64 else _lib.MX_F32
    dp, dj, dx, dB = Dev(p.astype(np.int32)), Dev(j.astype(np.int32)), Dev(x.astype(np.float64)), Dev(B_rowmajor)
    dC = Dev(nbytes=m * n * B_rowmajor.dtype.itemsize)
    check(lib.mx_dev_memset(dC.ptr, 0xFF, dC.nbytes, None))
    plan = C.c_void_p()
    check(lib.mxd_spmm_plan_create(m, K, dp.ptr, dj.ptr, dx.ptr, npanels, None, C.byref(plan)))
    try:
        check(lib.mxd_spmm_plan_run(plan, n, dB.ptr, n, dC.ptr, m if colmajor else n, dt, int(colmajor), wg_per_cu,
                                    sync_mode, None))
        check(lib.mx_stream_sync(None))
    finally:
        lib.mxd_spmm_plan_destroy(plan)
    out = dC.download(B_rowmajor.dtype, (n, m) if colmajor else (m, n))
    return out.T if colmajor else out


# ---------------------------------------------------------------------------------------------------------------------
# Guarded operands: B and C placed inside larger device buffers, so that a kernel that reads or writes outside its
# operand, or into the leading-dimension padding, is caught.
GUARD_BYTES = 4096
# bit patterns (quiet NaNs with a recognisable payload) that fill everything around an operand
SENTINEL = {np.dtype(np.float64): (np.uint64, 0x7FF8A5A55A5AC3C3), np.dtype(np.float32): (np.uint32, 0x7FC5A53C)}


class Guarded:
    """An `outer` x `inner` block at leading dimension `ld` (elements), `offset` elements into a device buffer with
    GUARD_BYTES of sentinel in front of the offset and behind the last row.  Every element outside the block holds
    the sentinel, or `pad` in the ld padding of each row when given.  `data` is None for an output block."""

    def __init__(self, dtype, outer, inner, ld, offset, data=None, pad=None):
        self.dtype = np.dtype(dtype)
        assert ld >= inner and offset >= 0
        self.outer, self.inner, self.ld = int(outer), int(inner), int(ld)
        isz = self.dtype.itemsize
        g = GUARD_BYTES // isz
        self.start = g + int(offset)
        total = self.start + self.outer * self.ld + g
        utype, bits = SENTINEL[self.dtype]
        host = np.empty(total, dtype=self.dtype)
        host.view(utype)[:] = utype(bits)
        block = host[self.start:self.start + self.outer * self.ld].reshape(self.outer, self.ld)
        if pad is not None:
            block[:, self.inner:] = pad
        if data is not None:
            assert data.shape == (self.outer, self.inner)
            block[:, :self.inner] = data
        self.expect = host
        self.buf = Dev(host)
        self.ptr = C.c_void_p(self.buf.ptr.value + self.start * isz)

    def _download(self):
        return self.buf.download(self.dtype, self.expect.shape)

    def _bits(self, a):
        return a.view(SENTINEL[self.dtype][0])

    def result(self):
        """The block, after asserting that every bit around it is what was uploaded."""
        got = self._download()
        inside = np.zeros(got.shape, dtype=bool)
        inside[self.start:self.start + self.outer * self.ld].reshape(self.outer, self.ld)[:, :self.inner] = True
        diff = np.flatnonzero((self._bits(got) != self._bits(self.expect)) & ~inside)
        assert diff.size == 0, (f"{diff.size} element(s) outside the {self.outer} x {self.inner} block (ld {self.ld}) "
                                f"changed, first at element {int(diff[0]) - self.start} relative to the block start")
        return got[self.start:self.start + self.outer * self.ld].reshape(self.outer, self.ld)[:, :self.inner].copy()

    def assert_untouched(self):
        got = self._download()
        diff = np.flatnonzero(self._bits(got) != self._bits(self.expect))
        assert diff.size == 0, f"{diff.size} element(s) of the buffer changed"


class DevCSR:
    """int32 indptr / indices and f64 values of a CSR matrix in device memory."""

    def __init__(self, p, j, x, K):
        self.m, self.K, self.nnz = int(p.size - 1), int(K), int(j.size)
        self.dp, self.dj, self.dx = Dev(p.astype(np.int32)), Dev(j.astype(np.int32)), Dev(x.astype(np.float64))


def last_kernel():
    return _lib.load().mxd_spmm_last_kernel().decode()


def plan_create(A, npanels=0, plan=None):
    """mxd_spmm_plan_create; pass a previous plan to rebuild it in place (its buffers are re-used)."""
    lib = _lib.load()
    handle = plan if plan is not None else C.c_void_p()
    check(lib.mxd_spmm_plan_create(A.m, A.K, A.dp.ptr, A.dj.ptr, A.dx.ptr, npanels, None, C.byref(handle)))
    return handle


def spmm_guarded(A, B, colmajor, algo=0, rows_sorted=False, npanels=0, wg_per_cu=0, plan=None, sync_mode=-1,
                 b_offset=0, ldb=None, c_offset=0, ldc=None):
    """C = A @ B with B (K x n, row-major) and C in guarded buffers: B at element offset `b_offset` with leading
    dimension `ldb` (NaN in the padding columns), C at `c_offset` with `ldc`.  Runs mxd_spmm_csr_dense_ex, or
    mxd_spmm_plan_run when a plan is given.  Returns (C as an (m, n) array, None) on success, (None, error message)
    when the call was refused; either way the guards, the padding and B must be unchanged."""
    lib = _lib.load()
    K, n = B.shape
    m = A.m
    ldb = n if ldb is None else ldb
    ldc = (m if colmajor else n) if ldc is None else ldc
    dt = _lib.MX_F64 if B.dtype == np.float64 else _lib.MX_F32
    gB = Guarded(B.dtype, K, n, ldb, b_offset, data=B, pad=np.nan)
    gC = Guarded(B.dtype, n if colmajor else m, m if colmajor else n, ldc, c_offset)
    if plan is None:
        rc = lib.mxd_spmm_csr_dense_ex(m, n, K, A.dp.ptr, A.dj.ptr, A.dx.ptr, gB.ptr, ldb, gC.ptr, ldc, dt,
                                       int(colmajor), algo, int(rows_sorted), npanels, wg_per_cu, None)
    else:
        rc = lib.mxd_spmm_plan_run(plan, n, gB.ptr, ldb, gC.ptr, ldc, dt, int(colmajor), wg_per_cu, sync_mode, None)
    err = None if rc == 0 else lib.mx_last_error().decode("utf-8", "replace")
    check(lib.mx_stream_sync(None))
    gB.assert_untouched()
    if err is not None:
        gC.assert_untouched()
        return None, err
    out = gC.result()
    return (out.T if colmajor else out), None


# ---------------------------------------------------------------------------------------------------------------------
# Guarded vectors and the device-level entries of the row-group kernels (one G-lane group per row: SpMV, merge,
# gather, column slices, cbind, sort, reverse-columns, CSR x / (.) vectors) and of the scan.  Every operand sits
# between GUARD_BYTES of sentinel; an output starts as poison, so that an element left unwritten, or written past
# the expected end, shows.
GUARD_PATTERN = np.array([0xA5, 0x5A, 0xC3, 0x3C], dtype=np.uint8)
# 8 bytes: a NaN with a payload as f64; as int32 / f32 halves 0x6B6B6B6B (no index, count or value used here) and a NaN
POISON_PATTERN = np.frombuffer(np.uint64(0x7FF8DEAD6B6B6B6B).tobytes(), dtype=np.uint8)
SLACK = 64                  # poisoned elements behind the expected end of an output


def last_row_launch():
    """(label, lanes per row) of the last row-group kernel launched"""
    return _lib.last_row_launch()


class GuardedVec:
    """n elements of `dtype` in device memory with GUARD_BYTES of sentinel on each side.  With `data` an input (or an
    in-place operand); without, an output of n elements pre-filled with poison."""

    def __init__(self, dtype, n=None, data=None):
        self.dtype = np.dtype(dtype)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=self.dtype).reshape(-1)
            n = data.size
        self.n, self.is_output = int(n), data is None
        isz = self.dtype.itemsize
        self.nbytes = -(-self.n * isz // 16) * 16                     # the payload region, padded to 16 B with poison
        host = np.tile(GUARD_PATTERN, (2 * GUARD_BYTES + self.nbytes) // 4)
        host[GUARD_BYTES:GUARD_BYTES + self.nbytes] = np.tile(POISON_PATTERN, self.nbytes // 8)
        if data is not None:
            host[GUARD_BYTES:GUARD_BYTES + self.n * isz] = data.view(np.uint8)
        self.expect = host
        self.buf = Dev(host)
        self.ptr = C.c_void_p(self.buf.ptr.value + GUARD_BYTES)

    def _download(self):
        got = self.buf.download(np.uint8, self.expect.shape)
        lo, hi = got[:GUARD_BYTES], got[GUARD_BYTES + self.nbytes:]
        for name, g, e in (("front", lo, self.expect[:GUARD_BYTES]), ("back", hi, self.expect[GUARD_BYTES + self.nbytes:])):
            diff = np.flatnonzero(g != e)
            assert diff.size == 0, f"{diff.size} byte(s) of the {name} guard changed, first at byte {int(diff[0])} of it"
        return got[GUARD_BYTES:GUARD_BYTES + self.nbytes]

    def _is_poison(self, payload):
        isz = self.dtype.itemsize
        want = np.tile(POISON_PATTERN, self.nbytes // 8)
        k = self.nbytes // isz
        return (payload.reshape(k, isz) == want.reshape(k, isz)).all(axis=1)

    def result(self, written=None):
        """The first `written` elements (default: all n), after asserting that the guards are bit-identical, that no
        poison is left among them and that everything behind them still is poison."""
        written = self.n if written is None else int(written)
        assert 0 <= written <= self.n
        payload = self._download()
        poison = self._is_poison(payload)
        left = np.flatnonzero(poison[:written])
        assert left.size == 0, f"{left.size} of {written} output element(s) never written, first at {int(left[0])}"
        stray = np.flatnonzero(~poison[written:])
        assert stray.size == 0, f"{stray.size} element(s) written past the end {written}, first at {written + int(stray[0])}"
        return payload[:written * self.dtype.itemsize].view(self.dtype).copy()

    def read(self):
        """All n elements of an in-place operand, after asserting that the guards and the padding are intact."""
        payload = self._download()
        tail = slice(self.n * self.dtype.itemsize, self.nbytes)
        assert np.array_equal(payload[tail], self.expect[GUARD_BYTES:GUARD_BYTES + self.nbytes][tail]), "padding changed"
        return payload[:self.n * self.dtype.itemsize].view(self.dtype).copy()

    def assert_untouched(self):
        got = self.buf.download(np.uint8, self.expect.shape)
        diff = np.flatnonzero(got != self.expect)
        assert diff.size == 0, f"{diff.size} byte(s) of an input buffer changed, first at byte {int(diff[0]) - GUARD_BYTES}"


_VAL_DTYPE = {_lib.MX_F64: np.float64, _lib.MX_F32: np.float32, _lib.MX_I32: np.int32, _lib.MX_LGL: np.int32}


class GCsr:
    """A CSR operand in guarded device memory: int32 indptr / indices, values of any dtype or none."""

    def __init__(self, p, j, x=None):
        self.m, self.nnz = int(p.size - 1), int(j.size)
        self.p, self.j = GuardedVec(np.int32, data=p), GuardedVec(np.int32, data=j)
        self.x = None if x is None else GuardedVec(np.asarray(x).dtype, data=x)
        self.xptr = None if x is None else self.x.ptr

    def assert_untouched(self):
        for g in (self.p, self.j, self.x):
            if g is not None:
                g.assert_untouched()


def _sync():
    check(_lib.load().mx_stream_sync(None))


def _untouched(*operands):
    for g in operands:
        if g is not None:
            g.assert_untouched()


def dev_spmv(A, v, v_dtype, hint):
    """mxd_spmv_csr_dvec: (y, launch)"""
    lib = _lib.load()
    gv = GuardedVec(_VAL_DTYPE[v_dtype], data=v)
    gy = GuardedVec(np.float32 if v_dtype == _lib.MX_F32 else np.float64, n=A.m)
    check(lib.mxd_spmv_csr_dvec(A.m, hint, A.p.ptr, A.j.ptr, A.xptr, gv.ptr, v_dtype, gy.ptr, None))
    _sync()
    launch = last_row_launch()
    _untouched(A, gv)
    return gy.result(), launch


def dev_merge(op, A, B, hint1, hint2):
    """mxd_csr_merge_count + _fill: (indptr, indices, values, total of the count pass, launches of both passes)"""
    lib = _lib.load()
    m = A.m
    vdt = np.int32 if op >= _lib.MX_OP_OR else np.float64
    gws = GuardedVec(np.uint8, n=lib.mxd_merge_workspace_bytes(m))
    gp = GuardedVec(np.int32, n=m + 1)
    total = C.c_int64(-1)
    check(lib.mxd_csr_merge_count(op, m, A.p.ptr, A.j.ptr, hint1, B.p.ptr, B.j.ptr, hint2, gp.ptr, gws.ptr,
                                  C.byref(total), None))
    launches = [last_row_launch()]
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(vdt, n=nout + SLACK)
    check(lib.mxd_csr_merge_fill(op, m, A.p.ptr, A.j.ptr, A.xptr, hint1, B.p.ptr, B.j.ptr, B.xptr, hint2, gp.ptr,
                                 gj.ptr, gx.ptr, None))
    _sync()
    launches.append(last_row_launch())
    _untouched(A, B)
    assert np.array_equal(gp.result(), indptr), "the fill pass changed out_indptr"
    return indptr, gj.result(nout), gx.result(nout), nout, launches


def _count_outputs(r):
    lib = _lib.load()
    return GuardedVec(np.uint8, n=lib.mxd_gather_workspace_bytes(r)), GuardedVec(np.int32, n=r + 1), C.c_int64(-1)


def dev_gather(A, rows, value_dtype, hint):
    """mxd_csr_gather_count + _fill: (indptr, indices, values or None, total, launch of the fill)"""
    lib = _lib.load()
    r = int(rows.size)
    grows = GuardedVec(np.int32, data=rows)
    gws, gp, total = _count_outputs(r)
    check(lib.mxd_csr_gather_count(r, A.p.ptr, grows.ptr, gp.ptr, gws.ptr, C.byref(total), None))
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj = GuardedVec(np.int32, n=nout + SLACK)
    gx = None if value_dtype == _lib.MX_NONE else GuardedVec(_VAL_DTYPE[value_dtype], n=nout + SLACK)
    check(lib.mxd_csr_gather_fill(r, A.p.ptr, A.j.ptr, A.xptr, grows.ptr, gp.ptr, gj.ptr,
                                  None if gx is None else gx.ptr, value_dtype, hint, None))
    _sync()
    launch = last_row_launch()
    _untouched(A, grows)
    assert np.array_equal(gp.result(), indptr), "the fill pass changed new_indptr"
    return indptr, gj.result(nout), None if gx is None else gx.result(nout), nout, launch


def dev_colrange(A, rows, min_col, max_col, value_dtype, avg):
    """mxd_csr_colrange_count + _fill: (indptr, indices, f64 values or None, total, launches of both passes)"""
    lib = _lib.load()
    r = int(rows.size)
    grows = GuardedVec(np.int32, data=rows)
    gws, gp, total = _count_outputs(r)
    check(lib.mxd_csr_colrange_count(r, A.p.ptr, A.j.ptr, grows.ptr, min_col, max_col, avg, gp.ptr, gws.ptr,
                                     C.byref(total), None))
    launches = [last_row_launch()]
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj = GuardedVec(np.int32, n=nout + SLACK)
    gx = None if value_dtype == _lib.MX_NONE else GuardedVec(np.float64, n=nout + SLACK)
    check(lib.mxd_csr_colrange_fill(r, A.p.ptr, A.j.ptr, A.xptr, value_dtype, grows.ptr, min_col, max_col, avg, gp.ptr,
                                    gj.ptr, None if gx is None else gx.ptr, None))
    _sync()
    launches.append(last_row_launch())
    _untouched(A, grows)
    assert np.array_equal(gp.result(), indptr), "the fill pass changed new_indptr"
    return indptr, gj.result(nout), None if gx is None else gx.result(nout), nout, launches


def dev_colmap(A, rows, cols, value_dtype, avg):
    """mxd_colmap_build + mxd_csr_colmap_count + _fill (rows are not re-sorted): (indptr, indices, values or None,
    total, launches of both passes)"""
    lib = _lib.load()
    r, ncol_map = int(rows.size), int(cols.max()) + 1
    grows, gcols = GuardedVec(np.int32, data=rows), GuardedVec(np.int32, data=cols)
    gstart, gpos = GuardedVec(np.int32, n=ncol_map + 1), GuardedVec(np.int32, n=cols.size)
    gmws = GuardedVec(np.uint8, n=lib.mxd_colmap_workspace_bytes(ncol_map))
    check(lib.mxd_colmap_build(gcols.ptr, cols.size, ncol_map, gstart.ptr, gpos.ptr, gmws.ptr, None))
    _sync()
    start, pos = gstart.result(), gpos.result()
    gmws._download()
    gws, gp, total = _count_outputs(r)
    check(lib.mxd_csr_colmap_count(r, A.p.ptr, A.j.ptr, grows.ptr, ncol_map, gstart.ptr, avg, gp.ptr, gws.ptr,
                                   C.byref(total), None))
    launches = [last_row_launch()]
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj = GuardedVec(np.int32, n=nout + SLACK)
    gx = None if value_dtype == _lib.MX_NONE else GuardedVec(_VAL_DTYPE[value_dtype], n=nout + SLACK)
    check(lib.mxd_csr_colmap_fill(r, A.p.ptr, A.j.ptr, A.xptr, value_dtype, grows.ptr, ncol_map, gstart.ptr, gpos.ptr,
                                  avg, gp.ptr, gj.ptr, None if gx is None else gx.ptr, None))
    _sync()
    launches.append(last_row_launch())
    _untouched(A, grows, gcols)
    assert np.array_equal(gstart.result(), start) and np.array_equal(gpos.result(), pos), "the column map changed"
    assert np.array_equal(gp.result(), indptr), "the fill pass changed new_indptr"
    return indptr, gj.result(nout), None if gx is None else gx.result(nout), nout, launches


def dev_cbind(X, Y, value_dtype, hint):
    """mxd_csr_cbind (Y's columns already shifted): (indptr, indices, values or None, launch)"""
    lib = _lib.load()
    nrows, nout = max(X.m, Y.m), X.nnz + Y.nnz
    gp, gj = GuardedVec(np.int32, n=nrows + 1), GuardedVec(np.int32, n=nout + SLACK)
    gx = None if value_dtype == _lib.MX_NONE else GuardedVec(_VAL_DTYPE[value_dtype], n=nout + SLACK)
    check(lib.mxd_csr_cbind(X.m, Y.m, X.p.ptr, X.j.ptr, X.xptr, Y.p.ptr, Y.j.ptr, Y.xptr, value_dtype, hint, gp.ptr,
                            gj.ptr, None if gx is None else gx.ptr, None))
    _sync()
    launch = last_row_launch()
    _untouched(X, Y)
    return gp.result(), gj.result(nout), None if gx is None else gx.result(nout), launch


def dev_sort_rows(A, value_dtype):
    """mxd_csr_sort_rows, in place on A's indices / values: (indices, values or None, launch)"""
    lib = _lib.load()
    gtj = GuardedVec(np.int32, n=A.nnz)
    gtx = None if value_dtype == _lib.MX_NONE else GuardedVec(_VAL_DTYPE[value_dtype], n=A.nnz)
    check(lib.mxd_csr_sort_rows(A.m, A.nnz, A.p.ptr, A.j.ptr, A.xptr, value_dtype, gtj.ptr,
                                None if gtx is None else gtx.ptr, None))
    _sync()
    launch = last_row_launch()
    A.p.assert_untouched()
    gtj.result()                      # every scratch entry written, none outside
    if gtx is not None:
        gtx.result()
    return A.j.read(), None if gtx is None else A.x.read(), launch


def dev_reverse_columns(A, value_dtype, ncol, hint):
    """mxd_csr_reverse_columns, in place: (indices, values or None, launch)"""
    lib = _lib.load()
    check(lib.mxd_csr_reverse_columns(A.m, hint, A.p.ptr, A.j.ptr, None if value_dtype == _lib.MX_NONE else A.xptr,
                                      value_dtype, ncol, None))
    _sync()
    launch = last_row_launch()
    A.p.assert_untouched()
    return A.j.read(), None if value_dtype == _lib.MX_NONE else A.x.read(), launch


def dev_spmv_svec(A, yi_base1, yv, kind, hint):
    """mxd_spmv_csr_svec: (out, launch)"""
    lib = _lib.load()
    gyi = GuardedVec(np.int32, data=yi_base1)
    gyv = None if yv is None else GuardedVec(np.asarray(yv).dtype, data=yv)
    gout = GuardedVec(np.float64, n=A.m)
    check(lib.mxd_spmv_csr_svec(A.m, hint, A.p.ptr, A.j.ptr, A.xptr, gyi.ptr, yi_base1.size,
                                None if gyv is None else gyv.ptr, kind, gout.ptr, None))
    _sync()
    launch = last_row_launch()
    _untouched(A, gyi, gyv)
    return gout.result(), launch


def dev_by_dvec(A, ncols, dvec, op, x_is_lhs, hint):
    """mxd_csr_by_dvec: (values_out, launch)"""
    lib = _lib.load()
    gd = GuardedVec(np.asarray(dvec).dtype, data=dvec)
    gout = GuardedVec(gd.dtype, n=A.nnz + SLACK)
    check(lib.mxd_csr_by_dvec(A.m, ncols, hint, A.p.ptr, A.j.ptr, A.xptr, gd.ptr, gd.n, op, int(x_is_lhs), gout.ptr,
                              None))
    _sync()
    launch = last_row_launch()
    _untouched(A, gd)
    return gout.result(A.nnz), launch


def dev_by_svec(A, ncol, vi_base1, vx, length, keep_na):
    """mxd_csr_by_svec_count + _fill: (indptr, indices, values, total, launches of both passes)"""
    lib = _lib.load()
    m = A.m
    gvi = GuardedVec(np.int32, data=vi_base1)
    gvx = None if vx is None else GuardedVec(np.float64, data=vx)
    vxp = None if gvx is None else gvx.ptr
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_by_svec_workspace_bytes(m))
    gp = GuardedVec(np.int32, n=m + 1)
    total, x_na = C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_csr_by_svec_count(m, ncol, A.nnz, A.p.ptr, A.xptr, gvi.ptr, vi_base1.size, vxp, length, int(keep_na),
                                    gws.ptr, gp.ptr, C.byref(total), C.byref(x_na), None))
    launches = [last_row_launch()]
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(np.float64, n=nout + SLACK)
    check(lib.mxd_csr_by_svec_fill(m, ncol, A.nnz, A.p.ptr, A.j.ptr, A.xptr, gvi.ptr, vi_base1.size, vxp, length,
                                   int(keep_na), gws.ptr, gp.ptr, gj.ptr, gx.ptr, None))
    _sync()
    launches.append(last_row_launch())
    _untouched(A, gvi, gvx)
    gws._download()
    return indptr, gj.result(nout), gx.result(nout), nout, launches


def dev_scan(counts):
    """mxd_exclusive_scan_i32: (out[n + 1], the int64 total)"""
    lib = _lib.load()
    n = int(counts.size)
    gc = GuardedVec(np.int32, data=counts)
    gout, gtotal = GuardedVec(np.int32, n=n + 1), GuardedVec(np.int64, n=1)
    gws = GuardedVec(np.uint8, n=lib.mxd_scan_workspace_bytes(n))
    check(lib.mxd_exclusive_scan_i32(gc.ptr, n, gout.ptr, gtotal.ptr, gws.ptr, None))
    _sync()
    gc.assert_untouched()
    gws._download()
    return gout.result(), int(gtotal.result()[0])


# ---------------------------------------------------------------------------------------------------------------------
# The two-pass families with a workspace of several segments (csrc/mx_workspace.h): every operand, every output and
# the workspace, exactly mxd_*_workspace_bytes long, between guards.  A segment that the library places past the size
# it publishes lands in the back guard.
def _ws(nbytes):
    return GuardedVec(np.uint8, n=nbytes)


def _entries(nout, *dtypes):
    return [None if dt is None else GuardedVec(dt, n=nout + SLACK) for dt in dtypes]


def _vec(a, dtype=None):
    return None if a is None else GuardedVec(np.asarray(a).dtype if dtype is None else dtype, data=a)


def _ptr(g):
    return None if g is None else g.ptr


def value_dtype_of(x):
    """MX_F64 for f64 values, MX_LGL for int32 ones, MX_NONE for none"""
    return _lib.MX_NONE if x is None else _lib.MX_F64 if np.asarray(x).dtype == np.float64 else _lib.MX_LGL


def dev_csc_dense_na(p, i, x, D, kind):
    """mxd_csc_dense_na_count + _fill of an m x n column-major D (dense kind 0..3): (indptr, indices, values)"""
    lib = _lib.load()
    m, n = D.shape
    A, gd = GCsr(p, i, x), GuardedVec(D.dtype, data=np.asarray(D).reshape(-1, order="F"))
    gws = _ws(lib.mxd_csc_dense_na_workspace_bytes(m, n))
    total, outside = C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_csc_dense_na_count(m, n, A.nnz, A.p.ptr, A.j.ptr, gd.ptr, kind, gws.ptr, C.byref(total),
                                     C.byref(outside), None))
    gws._download()
    nout = int(total.value)
    gp = GuardedVec(np.int32, n=n + 1)
    gj, gx = _entries(nout, np.int32, np.float64)
    check(lib.mxd_csc_dense_na_fill(m, n, A.nnz, A.p.ptr, A.j.ptr, A.xptr, gd.ptr, kind, gws.ptr, gp.ptr, gj.ptr, gx.ptr,
                                    None))
    _sync()
    _untouched(A, gd)
    gws._download()
    return gp.result(), gj.result(nout), gx.result(nout)


def dev_dvec_na_rows(p, j, x, ncols, v, op):
    """mxd_csr_by_dvec_na_rows_count + _fill (the vector's length divides the rows): dict(indptr, indices, values)"""
    lib = _lib.load()
    A, gv, m, code = GCsr(p, j, x), GuardedVec(np.float64, data=v), int(p.size - 1), _lib.MX_DV_OPS[op]
    gws, gp, total = _ws(lib.mxd_csr_by_dvec_na_rows_workspace_bytes(m)), GuardedVec(np.int32, n=m + 1), C.c_int64(-1)
    check(lib.mxd_csr_by_dvec_na_rows_count(m, ncols, A.nnz, A.p.ptr, gv.ptr, gv.n, code, gws.ptr, gp.ptr,
                                            C.byref(total), None))
    gws._download()
    nout = int(total.value)
    gj, gx = _entries(nout, np.int32, np.float64)
    check(lib.mxd_csr_by_dvec_na_rows_fill(m, ncols, A.nnz, A.p.ptr, A.j.ptr, A.xptr, gv.ptr, gv.n, code, gp.ptr, gj.ptr,
                                           gx.ptr, None))
    _sync()
    _untouched(A, gv)
    return dict(indptr=gp.result(), indices=gj.result(nout), values=gx.result(nout))


def dev_dvec_na_flat(p, j, x, ncols, v, op):
    """The flat route of the NA-keeping CSR (op) dense vector, step by step as device.csr_by_dvec_keep_na takes it:
    mxd_dvec_na_special, mxd_dvec_na_cells_count / _fill, the new cells through mxd_coo_to_csr, mxd_csr_join_disjoint.
    Returns (dict(indptr, indices, values), special positions, candidate cells, new cells)."""
    lib = _lib.load()
    A, gv, m, code = GCsr(p, j, x), GuardedVec(np.float64, data=v), int(p.size - 1), _lib.MX_DV_OPS[op]
    L = gv.n
    sws = _ws(lib.mxd_dvec_na_special_workspace_bytes(L))
    nsp, cand, new = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_dvec_na_special(m, ncols, gv.ptr, L, code, sws.ptr, C.byref(nsp), C.byref(cand), None))
    sws._download()
    assert cand.value > 0, "the case has no candidate cell"
    cws = _ws(lib.mxd_dvec_na_cells_workspace_bytes(cand.value))
    check(lib.mxd_dvec_na_cells_count(m, ncols, A.nnz, A.p.ptr, A.j.ptr, L, sws.ptr, nsp.value, cand.value, cws.ptr,
                                      C.byref(new), None))
    cws._download()
    n_new = int(new.value)
    assert n_new > 0, "the case adds no cell"
    gax = GuardedVec(np.float64, n=A.nnz + SLACK)
    check(lib.mxd_csr_by_dvec(m, ncols, A.nnz, A.p.ptr, A.j.ptr, A.xptr, gv.ptr, L, code, 1, gax.ptr, None))
    gi, gj, gx = _entries(n_new, np.int32, np.int32, np.float64)
    check(lib.mxd_dvec_na_cells_fill(m, ncols, gv.ptr, L, code, sws.ptr, nsp.value, cand.value, cws.ptr, gi.ptr, gj.ptr,
                                     gx.ptr, None))
    _sync()
    sws._download()
    cws._download()
    bp, bj, bx = dev_coo_to_csr(gi.result(n_new), gj.result(n_new), gx.result(n_new), m, ncols)
    assert bj.size == n_new, "the new cells are not distinct"
    B = GCsr(bp, bj, bx)
    nout = A.nnz + n_new
    gp = GuardedVec(np.int32, n=m + 1)
    oj, ox = _entries(nout, np.int32, np.float64)
    check(lib.mxd_csr_join_disjoint(m, A.p.ptr, A.j.ptr, gax.ptr, A.nnz, B.p.ptr, B.j.ptr, B.xptr, n_new, gp.ptr, oj.ptr,
                                    ox.ptr, None))
    _sync()
    _untouched(A, B, gv)
    gax.result(A.nnz)
    return (dict(indptr=gp.result(), indices=oj.result(nout), values=ox.result(nout)), int(nsp.value), int(cand.value),
            n_new)


def dev_dense_by_svec(X, kind, vi_base1, vx, length, keep_na):
    """mxd_dense_by_svec_dense (the routes with a dense result: dict(X_dense)) or mxd_dense_by_svec_count + _fill
    (dict(indptr, indices, values)), as mx_dense_by_svec_route chooses; X column-major, dense kind 0..3"""
    lib = _lib.load()
    nrows, ncols = X.shape
    gX = GuardedVec(X.dtype, data=np.asarray(X).reshape(-1, order="F"))
    gvi, gvx = GuardedVec(np.int32, data=vi_base1), GuardedVec(np.float64, data=vx)
    nv, keep = gvi.n, int(bool(keep_na))
    route = lib.mx_dense_by_svec_route(nrows, ncols, length)
    assert route >= 0
    if route in (_lib.MX_DSV_ROUTE_A, _lib.MX_DSV_ROUTE_D):
        gws, gout = _ws(lib.mxd_dense_by_svec_workspace_bytes(0, length)), GuardedVec(np.float64, n=nrows * ncols)
        check(lib.mxd_dense_by_svec_dense(nrows, ncols, gX.ptr, kind, gvi.ptr, nv, gvx.ptr, length, keep, gws.ptr,
                                          gout.ptr, None))
        _sync()
        _untouched(gX, gvi, gvx)
        gws._download()
        return dict(X_dense=gout.result().reshape((nrows, ncols), order="F"))
    gws, gp, total = _ws(lib.mxd_dense_by_svec_workspace_bytes(nrows, length)), GuardedVec(np.int32, n=nrows + 1), C.c_int64(-1)
    check(lib.mxd_dense_by_svec_count(nrows, ncols, gX.ptr, kind, gvi.ptr, nv, length, keep, gws.ptr, gp.ptr,
                                      C.byref(total), None))
    gws._download()
    nout = int(total.value)
    gj, gx = _entries(nout, np.int32, np.float64)
    check(lib.mxd_dense_by_svec_fill(nrows, ncols, gX.ptr, kind, gvx.ptr, length, keep, gws.ptr, gp.ptr, gj.ptr, gx.ptr,
                                     None))
    _sync()
    _untouched(gX, gvi, gvx)
    gws._download()
    return dict(indptr=gp.result(), indices=gj.result(nout), values=gx.result(nout))


def dev_outer_dense(p, x, colvec):
    """mxd_csr_outer_dense_count + _fill of a one-column CSR (p, x) and an f64 / f32 vector: dict(indptr, indices, values)"""
    lib = _lib.load()
    m, dim = int(p.size - 1), int(colvec.size)
    gp_in, gx_in, gv = GuardedVec(np.int32, data=p), GuardedVec(np.float64, data=x), GuardedVec(colvec.dtype, data=colvec)
    gws, gp, total = _ws(lib.mxd_csr_outer_dense_workspace_bytes(m)), GuardedVec(np.int32, n=m + 1), C.c_int64(-1)
    check(lib.mxd_csr_outer_dense_count(m, dim, gp_in.ptr, gws.ptr, gp.ptr, C.byref(total), None))
    gws._download()
    nout = int(total.value)
    gj, gx = _entries(nout, np.int32, np.float64)
    check(lib.mxd_csr_outer_dense_fill(m, dim, gx_in.n, gp_in.ptr, gx_in.ptr, gv.ptr,
                                       _lib.MX_F64 if colvec.dtype == np.float64 else _lib.MX_F32, gp.ptr, gj.ptr, gx.ptr,
                                       None))
    _sync()
    _untouched(gp_in, gx_in, gv)
    return dict(indptr=gp.result(), indices=gj.result(nout), values=gx.result(nout))


def dev_outer_svec(p, x, yi_base1, yv, v_dtype, length):
    """mxd_csr_outer_svec_count + _fill of a one-column CSR (p, x) and a sparse vector: dict(indptr, indices, values)"""
    lib = _lib.load()
    m = int(p.size - 1)
    gp_in, gx_in = GuardedVec(np.int32, data=p), GuardedVec(np.float64, data=x)
    gyi, gyv = GuardedVec(np.int32, data=yi_base1), _vec(yv)
    gws, gp = _ws(lib.mxd_csr_outer_svec_workspace_bytes(m, length)), GuardedVec(np.int32, n=length + 1)
    nonempty, total = C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_csr_outer_svec_count(m, gx_in.n, gp_in.ptr, gx_in.ptr, gyi.ptr, gyi.n, length, gws.ptr, gp.ptr,
                                       C.byref(nonempty), C.byref(total), None))
    gws._download()
    nout = int(total.value)
    gi, gx = _entries(nout, np.int32, np.float64)
    check(lib.mxd_csr_outer_svec_fill(m, gyi.ptr, gyi.n, _ptr(gyv), v_dtype, length, nonempty.value, gws.ptr, gp.ptr,
                                      gi.ptr, gx.ptr, None))
    _sync()
    _untouched(gp_in, gx_in, gyi, gyv)
    gws._download()
    return dict(indptr=gp.result(), indices=gi.result(nout), values=gx.result(nout))


def dev_coo_slice(i, j, x, m, n, rows_take_base1, col_lo, col_hi):
    """mxd_coo_slice_count + _fill with a map on the rows (mxd_colmap_build of the 1-based selector, repeats allowed)
    and the columns col_lo..col_hi: (rows, cols, values or None) of the slice"""
    lib = _lib.load()
    gi, gj, gx = GuardedVec(np.int32, data=i), GuardedVec(np.int32, data=j), _vec(x)
    vd, nnz = value_dtype_of(x), gi.n
    gtake = GuardedVec(np.int32, data=rows_take_base1)
    nmap = int(np.max(rows_take_base1)) + 1
    gstart, gpos = GuardedVec(np.int32, n=nmap + 1), GuardedVec(np.int32, n=gtake.n)
    gmws = _ws(lib.mxd_colmap_workspace_bytes(nmap))
    check(lib.mxd_colmap_build(gtake.ptr, gtake.n, nmap, gstart.ptr, gpos.ptr, gmws.ptr, None))
    _sync()
    gmws._download()
    ai = _lib.CooAxis(1, 0, 0, 0, nmap, gstart.ptr.value, gpos.ptr.value)
    aj = _lib.CooAxis(0, col_lo, col_hi, 0, 0, None, None)
    gws, total = _ws(lib.mxd_coo_slice_workspace_bytes(nnz)), C.c_int64(-1)
    check(lib.mxd_coo_slice_count(m, n, gi.ptr, gj.ptr, nnz, C.byref(ai), C.byref(aj), gws.ptr, C.byref(total), None))
    gws._download()
    nout = int(total.value)
    oi, oj, ox = _entries(nout, np.int32, np.int32, None if x is None else x.dtype)
    check(lib.mxd_coo_slice_fill(m, n, gi.ptr, gj.ptr, _ptr(gx), vd, nnz, C.byref(ai), C.byref(aj), gws.ptr, oi.ptr,
                                 oj.ptr, _ptr(ox), None))
    _sync()
    _untouched(gi, gj, gx, gtake)
    gws._download()
    gstart.result(), gpos.result()
    return oi.result(nout), oj.result(nout), None if ox is None else ox.result(nout)


def dev_coo_single(i, j, x, r, c):
    """mxd_coo_single: (index of the first triplet at (r, c) or -1, the 8 value bytes read back)"""
    lib = _lib.load()
    gi, gj, gx = GuardedVec(np.int32, data=i), GuardedVec(np.int32, data=j), _vec(x)
    gws, k, value = _ws(lib.mxd_coo_single_workspace_bytes()), C.c_int64(-2), (C.c_uint8 * 8)()
    check(lib.mxd_coo_single(gi.ptr, gj.ptr, _ptr(gx), value_dtype_of(x), gi.n, r, c, gws.ptr, C.byref(k), value, None))
    _sync()
    _untouched(gi, gj, gx)
    gws._download()
    return int(k.value), bytes(value)


def dev_csr_by_coo(logical, p, j, x, ncol, yi, yj, yv):
    """mxd_csr_by_coo_count + _fill: (rows, cols, values) in the order of y's entries"""
    lib = _lib.load()
    A, m = GCsr(p, j, x), int(p.size - 1)
    gyi, gyj, gyv = GuardedVec(np.int32, data=yi), GuardedVec(np.int32, data=yj), _vec(yv)
    gws, total = _ws(lib.mxd_csr_by_coo_workspace_bytes(gyi.n)), C.c_int64(-1)
    check(lib.mxd_csr_by_coo_count(int(logical), m, ncol, A.p.ptr, A.j.ptr, A.xptr, gyi.ptr, gyj.ptr, gyv.ptr, gyi.n,
                                   gws.ptr, C.byref(total), None))
    gws._download()
    nout = int(total.value)
    oi, oj, ox = _entries(nout, np.int32, np.int32, gyv.dtype)
    check(lib.mxd_csr_by_coo_fill(int(logical), m, ncol, A.p.ptr, A.j.ptr, A.xptr, gyi.ptr, gyj.ptr, gyv.ptr, gyi.n,
                                  gws.ptr, oi.ptr, oj.ptr, ox.ptr, None))
    _sync()
    _untouched(A, gyi, gyj, gyv)
    gws._download()
    return oi.result(nout), oj.result(nout), ox.result(nout)


def dev_compact(p, j, x, rule, mask=None):
    """mxd_compact_count + _fill over the entries of a CSR: (indptr, indices, values, kept)"""
    lib = _lib.load()
    A, gmask, vd, m = GCsr(p, j, x), _vec(mask, np.int32), value_dtype_of(x), int(p.size - 1)
    gws, kept = _ws(lib.mxd_compact_workspace_bytes(A.nnz)), C.c_int64(-1)
    check(lib.mxd_compact_count(A.nnz, A.xptr, vd, rule, _ptr(gmask), gws.ptr, C.byref(kept), None))
    gws._download()
    nout = int(kept.value)
    gp = GuardedVec(np.int32, n=m + 1)
    oj, ox = _entries(nout, np.int32, A.x.dtype)
    check(lib.mxd_compact_fill(A.nnz, A.xptr, vd, rule, _ptr(gmask), A.j.ptr, None, m, A.p.ptr, gws.ptr, oj.ptr, None,
                               ox.ptr, gp.ptr, None))
    _sync()
    _untouched(A, gmask)
    gws._download()
    return gp.result(), oj.result(nout), ox.result(nout), nout


def dev_csr_transpose(p, j, x, ncol):
    """mxd_csr_transpose: (indptr, indices, values or None) of the transpose, repeated cells merged"""
    lib = _lib.load()
    A = GCsr(p, j, x)
    gws, total = _ws(lib.mxd_csr_transpose_workspace_bytes(A.nnz)), C.c_int64(-1)
    gp = GuardedVec(np.int32, n=ncol + 1)
    oj, ox = _entries(A.nnz, np.int32, None if x is None else x.dtype)
    check(lib.mxd_csr_transpose(A.m, ncol, A.p.ptr, A.j.ptr, A.xptr, value_dtype_of(x), A.nnz, gp.ptr, oj.ptr, _ptr(ox),
                                gws.ptr, C.byref(total), None))
    _sync()
    _untouched(A)
    gws._download()
    nout = int(total.value)        # every entry is written before repeated cells are merged into the first nout
    return gp.result(), oj.result(A.nnz)[:nout], None if ox is None else ox.result(A.nnz)[:nout]


def dev_coo_to_csr(i, j, x, m, n):
    """mxd_coo_to_csr: (indptr, indices, values or None), repeated cells merged"""
    lib = _lib.load()
    gi, gj, gx = GuardedVec(np.int32, data=i), GuardedVec(np.int32, data=j), _vec(x)
    nnz = gi.n
    gws, total = _ws(lib.mxd_coo_to_csr_workspace_bytes(nnz, n)), C.c_int64(-1)
    gp = GuardedVec(np.int32, n=m + 1)
    oj, ox = _entries(nnz, np.int32, None if x is None else x.dtype)
    check(lib.mxd_coo_to_csr(m, n, gi.ptr, gj.ptr, _ptr(gx), value_dtype_of(x), nnz, gp.ptr, oj.ptr, _ptr(ox), gws.ptr,
                             C.byref(total), None))
    _sync()
    _untouched(gi, gj, gx)
    gws._download()
    nout = int(total.value)        # every entry is written before repeated cells are merged into the first nout
    return gp.result(), oj.result(nnz)[:nout], None if ox is None else ox.result(nnz)[:nout]


def dev_sort_vector(ii, xx, value_dtype):
    """mxd_sort_vector_indices, in place: (indices, values or None, was_sorted)"""
    lib = _lib.load()
    gi, gx = GuardedVec(np.int32, data=ii), _vec(xx)
    gws, was = _ws(lib.mxd_sort_vector_indices_workspace_bytes(gi.n)), C.c_int(-1)
    check(lib.mxd_sort_vector_indices(gi.ptr, _ptr(gx), gi.n, value_dtype, gws.ptr, C.byref(was), None))
    _sync()
    gws._download()
    return gi.read(), None if gx is None else gx.read(), int(was.value)
