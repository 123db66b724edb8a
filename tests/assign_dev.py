"""Test helper: the device-level entries of the CSR assignment (mxd_csr_assign_* / mxd_csr_replace_rows_*, assign.hip)
with every operand, every output, the selector maps and the workspace between guards (tests/devmem.py)."""
import ctypes as C

import numpy as np

from devmem import SLACK, GuardedVec, _sync, _untouched, last_row_launch
from matrixextra_amd import _lib
from matrixextra_amd._lib import check


class Axis:
    """An mx_coo_axis of a 0-based selector: None (all of n), ("range", lo, hi[, reversed]) or ("set", indices).  An
    arbitrary set becomes the dense map mxd_colmap_build makes of the 1-based selector, in guarded memory."""

    def __init__(self, sel, n):
        self.guards = []
        if sel is None or sel[0] == "range":
            lo, hi = (0, n - 1) if sel is None else sel[1:3]
            self.n = hi - lo + 1
            self.c = _lib.CooAxis(_lib.MX_AXIS_AFFINE, lo, hi, int(sel[3]) if sel is not None and len(sel) > 3 else 0, 0,
                                  None, None)
            self.members = np.arange(lo, hi + 1)
            return
        lib = _lib.load()
        idx = np.asarray(sel[1], dtype=np.int32)
        self.n, self.members = idx.size, idx
        nmap = int(idx.max()) + 2
        gtake = GuardedVec(np.int32, data=idx + 1)
        gstart, gpos = GuardedVec(np.int32, n=nmap + 1), GuardedVec(np.int32, n=idx.size)
        gws = GuardedVec(np.uint8, n=lib.mxd_colmap_workspace_bytes(nmap))
        check(lib.mxd_colmap_build(gtake.ptr, idx.size, nmap, gstart.ptr, gpos.ptr, gws.ptr, None))
        _sync()
        gws._download()
        gtake.assert_untouched()
        self.start, self.pos = gstart.result(), gpos.result()
        self.gsorted = GuardedVec(np.int32, data=np.sort(idx))
        self.guards = [gstart, gpos, self.gsorted]
        self.c = _lib.CooAxis(_lib.MX_AXIS_MAP, 0, 0, 0, nmap, gstart.ptr.value, gpos.ptr.value)

    def sorted_ptr(self):
        return self.gsorted.ptr if self.guards else None

    def assert_untouched(self):
        if self.guards:
            assert np.array_equal(self.guards[0].result(), self.start) and np.array_equal(self.guards[1].result(), self.pos)
            self.gsorted.assert_untouched()


def _count_outputs(nrows):
    lib = _lib.load()
    return (GuardedVec(np.uint8, n=lib.mxd_gather_workspace_bytes(nrows)), GuardedVec(np.int32, n=nrows + 1),
            C.c_int64(-1))


def dev_assign_scalar(A, ncols, rows, cols, value, avg):
    """mxd_csr_assign_count + _fill: (indptr, indices, values, total, hits, launches of both passes)"""
    lib = _lib.load()
    m = A.m
    ai, aj = Axis(rows, m), Axis(cols, ncols)
    is_const = int(not value == 0)
    gws, gp, total = _count_outputs(m)
    hits = C.c_int64(-1)
    check(lib.mxd_csr_assign_count(m, ncols, A.p.ptr, A.j.ptr, A.nnz, C.byref(ai.c), C.byref(aj.c), ai.n, aj.n, is_const,
                                   avg, gp.ptr, gws.ptr, C.byref(total), C.byref(hits), None))
    launches = [last_row_launch()]
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(np.float64, n=nout + SLACK)
    check(lib.mxd_csr_assign_fill(m, ncols, A.p.ptr, A.j.ptr, A.xptr, C.byref(ai.c), C.byref(aj.c), aj.sorted_ptr(), aj.n,
                                  is_const, float(value), avg, gp.ptr, gj.ptr, gx.ptr, None))
    _sync()
    launches.append(last_row_launch())
    _untouched(A)
    ai.assert_untouched()
    aj.assert_untouched()
    assert np.array_equal(gp.result(), indptr), "the fill pass changed new_indptr"
    return indptr, gj.result(nout), gx.result(nout), nout, int(hits.value), launches


def dev_replace_rows(A, rows, V, avg):
    """mxd_csr_replace_rows_count + _fill: (indptr, indices, values, total, launch of the fill)"""
    lib = _lib.load()
    m = A.m
    ai = Axis(rows, m)
    gws, gp, total = _count_outputs(m)
    check(lib.mxd_csr_replace_rows_count(m, A.p.ptr, C.byref(ai.c), V.m, V.p.ptr, gp.ptr, gws.ptr, C.byref(total), None))
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj, gx = GuardedVec(np.int32, n=nout + SLACK), GuardedVec(np.float64, n=nout + SLACK)
    check(lib.mxd_csr_replace_rows_fill(m, A.p.ptr, A.j.ptr, A.xptr, C.byref(ai.c), V.m, V.p.ptr, V.j.ptr, V.xptr, avg,
                                        gp.ptr, gj.ptr, gx.ptr, None))
    _sync()
    launch = last_row_launch()
    _untouched(A, V)
    ai.assert_untouched()
    assert np.array_equal(gp.result(), indptr), "the fill pass changed new_indptr"
    return indptr, gj.result(nout), gx.result(nout), nout, launch
