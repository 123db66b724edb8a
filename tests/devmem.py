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
