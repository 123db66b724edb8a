"""Test helper: the device-level entries of the vector-valued CSR assignment (mxd_csr_assign_col_* and
mxd_csr_expand_pattern_row, assignvec.hip) with every operand, every output, the pattern and the workspace between
guards (tests/devmem.py)."""
import ctypes as C

import numpy as np

from devmem import SLACK, GuardedVec, _sync, _untouched, last_row_launch
from matrixextra_amd import _lib
from matrixextra_amd._lib import check


class Pattern:
    """(ii, xx, length) in guarded device memory; ii None for a dense vector.  A sparse pattern without entries keeps
    a non-null ii."""

    def __init__(self, ii, xx, length):
        self.gii = None if ii is None else GuardedVec(np.int32, data=np.asarray(ii, dtype=np.int32))
        self.gxx = GuardedVec(np.float64, data=np.asarray(xx, dtype=np.float64))
        self.n, self.length = self.gxx.n, int(length)
        self.ii_ptr = None if self.gii is None else self.gii.ptr

    def assert_untouched(self):
        _untouched(self.gii, self.gxx)


def dev_assign_col(A, ncols, col, pat, avg, values_only=False):
    """mxd_csr_assign_col_count + _fill: (indptr, indices or None, values, total, changed, launches of both passes).
    values_only: the fill gets no new_indices and the input's indptr, which wants changed == 0."""
    lib = _lib.load()
    m = A.m
    gws, gp = GuardedVec(np.uint8, n=lib.mxd_gather_workspace_bytes(m)), GuardedVec(np.int32, n=m + 1)
    total, changed = C.c_int64(-1), C.c_int64(-1)
    check(lib.mxd_csr_assign_col_count(m, ncols, A.p.ptr, A.j.ptr, A.nnz, col, pat.ii_ptr, pat.n, pat.length, avg,
                                       gp.ptr, gws.ptr, C.byref(total), C.byref(changed), None))
    launches = [last_row_launch()]
    indptr = gp.result()
    gws._download()
    nout = int(total.value)
    gj = None if values_only else GuardedVec(np.int32, n=nout + SLACK)
    gx = GuardedVec(np.float64, n=nout + SLACK)
    if values_only:
        assert changed.value == 0 and nout == A.nnz
    check(lib.mxd_csr_assign_col_fill(m, ncols, A.p.ptr, A.j.ptr, A.xptr, col, pat.ii_ptr, pat.gxx.ptr, pat.n,
                                      pat.length, avg, A.p.ptr if values_only else gp.ptr,
                                      None if values_only else gj.ptr, gx.ptr, None))
    _sync()
    launches.append(last_row_launch())
    _untouched(A)
    pat.assert_untouched()
    gws._download()
    assert np.array_equal(gp.result(), indptr), "the fill pass changed new_indptr"
    return indptr, None if gj is None else gj.result(nout), gx.result(nout), nout, int(changed.value), launches


def dev_expand_pattern(pat, n_repeats, values_only=False):
    """mxd_csr_expand_pattern_row: (row_indptr or None, row_indices or None, row_values)"""
    lib = _lib.load()
    total = pat.n * n_repeats
    gp = None if values_only else GuardedVec(np.int32, n=2)
    gj = None if values_only else GuardedVec(np.int32, n=total + SLACK)
    gx = GuardedVec(np.float64, n=total + SLACK)
    check(lib.mxd_csr_expand_pattern_row(pat.ii_ptr, pat.gxx.ptr, pat.n, pat.length, n_repeats,
                                         None if gp is None else gp.ptr, None if gj is None else gj.ptr, gx.ptr, None))
    _sync()
    pat.assert_untouched()
    return (None if gp is None else gp.result(), None if gj is None else gj.result(total), gx.result(total))
