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
        check(lib.mx_dev_malloc(C.byref(self.ptr), C.c_size_t(max(self.nbytes, 16))))
        if self.host is not None and self.nbytes:
            check(lib.mx_memcpy_h2d(self.ptr, C.c_void_p(self.host.ctypes.data), C.c_size_t(self.nbytes), None))
            check(lib.mx_stream_sync(None))

    def download(self, dtype, shape):
        lib = _lib.load()
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            check(lib.mx_memcpy_d2h(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(out.nbytes), None))
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
    check(lib.mx_dev_memset(dC.ptr, 0xFF, C.c_size_t(dC.nbytes), None))      # poison: every element must be written
    check(lib.mxd_spmm_csr_dense_ex(C.c_int(m), C.c_int(n), C.c_int(K), dp.ptr, dj.ptr, dx.ptr, dB.ptr, C.c_size_t(n),
                                    dC.ptr, C.c_size_t(m if colmajor else n), C.c_int(dt), C.c_int(int(colmajor)),
                                    C.c_int(algo), C.c_int(int(rows_sorted)), C.c_int(npanels), C.c_int(wg_per_cu), None))
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
    check(lib.mx_dev_memset(dC.ptr, 0xFF, C.c_size_t(dC.nbytes), None))
    plan = C.c_void_p()
    check(lib.mxd_spmm_plan_create(C.c_int(m), C.c_int(K), dp.ptr, dj.ptr, dx.ptr, C.c_int(npanels), None, C.byref(plan)))
    try:
        check(lib.mxd_spmm_plan_run(plan, C.c_int(n), dB.ptr, C.c_size_t(n), dC.ptr, C.c_size_t(m if colmajor else n),
                                    C.c_int(dt), C.c_int(int(colmajor)), C.c_int(wg_per_cu), C.c_int(sync_mode), None))
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
    check(lib.mxd_spmm_plan_create(C.c_int(A.m), C.c_int(A.K), A.dp.ptr, A.dj.ptr, A.dx.ptr, C.c_int(npanels), None,
                                   C.byref(handle)))
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
        rc = lib.mxd_spmm_csr_dense_ex(C.c_int(m), C.c_int(n), C.c_int(K), A.dp.ptr, A.dj.ptr, A.dx.ptr, gB.ptr,
                                       C.c_size_t(ldb), gC.ptr, C.c_size_t(ldc), C.c_int(dt), C.c_int(int(colmajor)),
                                       C.c_int(algo), C.c_int(int(rows_sorted)), C.c_int(npanels), C.c_int(wg_per_cu),
                                       None)
    else:
        rc = lib.mxd_spmm_plan_run(plan, C.c_int(n), gB.ptr, C.c_size_t(ldb), gC.ptr, C.c_size_t(ldc), C.c_int(dt),
                                   C.c_int(int(colmajor)), C.c_int(wg_per_cu), C.c_int(sync_mode), None)
    err = None if rc == 0 else lib.mx_last_error().decode("utf-8", "replace")
    check(lib.mx_stream_sync(None))
    gB.assert_untouched()
    if err is not None:
        gC.assert_untouched()
        return None, err
    out = gC.result()
    return (out.T if colmajor else out), None
