"""Operands for the rbind / cbind tests and the guarded-buffer drivers of the device entries they add
(mxd_csr_rbind_batch, mxd_coo_rbind_append, mxd_csr_cbind_svec).  An operand is the tuple the oracle and
exports.concat_csr_batch take: (kind, indptr | None, indices, values | None, nrows), kinds 0 dgR, 1 lgR, 2 ngR,
3 / 4 / 5 / 6 d / i / l / n sparseVector (1-based indices, one row)."""
import ctypes as C

import numpy as np

from devmem import SLACK, GuardedVec, _sync
from matrixextra_amd import _lib
from matrixextra_amd._lib import check

NA = -2147483648
TILE = 1024            # output entries per workgroup of the entry pass (RBIND_TILE in csrc/bind.hip)
STAGE = 2048           # entry offsets a spanning tile keeps in LDS (RBIND_STAGE); a wider span searches the table


def values_of(kind, n, rng):
    """n values of an operand kind with 0, NA / NaN among them (None for the pattern kinds)"""
    if kind in (2, 6):
        return None
    if kind in (0, 3):
        v = np.round(rng.normal(size=n), 2)
        v[rng.random(n) < 0.15] = 0.0
        v[rng.random(n) < 0.15] = np.nan
        return v
    if kind == 4:
        v = rng.integers(-3, 4, size=n).astype(np.int32)
    else:
        v = rng.integers(0, 2, size=n).astype(np.int32)
    v[rng.random(n) < 0.2] = NA
    return v


def matrix(kind, nrows, ncol, rng, density=0.5):
    mask = rng.random((nrows, ncol)) < density
    p = np.zeros(nrows + 1, np.int32)
    p[1:] = np.cumsum(mask.sum(axis=1))
    j = np.nonzero(mask)[1].astype(np.int32)
    return (kind, p, j, values_of(kind, j.size, rng), nrows)


def matrix_of_nnz(kind, nnz, ncol, rng):
    """full rows of ncol entries, then one shorter row: exactly nnz entries"""
    lens = [ncol] * (nnz // ncol) + ([nnz % ncol] if nnz % ncol else [])
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = np.concatenate([np.arange(n) for n in lens] + [np.zeros(0, int)]).astype(np.int32)
    return (kind, p, j, values_of(kind, nnz, rng), len(lens))


def vector(kind, n, ncol, rng):
    i = (np.sort(rng.permutation(ncol)[:n]) + 1).astype(np.int32)
    return (kind, None, i, values_of(kind, n, rng), 1)


def empty_rows(kind, nrows):
    """a matrix with rows and no entry (nrows = 0: no rows either)"""
    return (kind, np.zeros(nrows + 1, np.int32), np.zeros(0, np.int32),
            None if kind == 2 else np.zeros(0, np.float64 if kind == 0 else np.int32), nrows)


def nnz_of(objs):
    return sum(int(np.asarray(o[2]).size) for o in objs)


def same_values(got, want):
    """exact, NaN-ness compared (tests/test_gpu_parity.py::assert_list_equal)"""
    if want is None:
        assert got is None
        return
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype.kind == "f":
        nan_g, nan_w = np.isnan(got), np.isnan(want)
        np.testing.assert_array_equal(nan_g, nan_w)
        np.testing.assert_array_equal(got[~nan_g].view(np.int64), want[~nan_w].view(np.int64))
    else:
        np.testing.assert_array_equal(got, want)


def same_csr(got, want):
    assert got["indptr"].dtype == np.int32 and got["indices"].dtype == np.int32
    np.testing.assert_array_equal(got["indptr"], want["indptr"])
    np.testing.assert_array_equal(got["indices"], want["indices"])
    same_values(got["values"], want["values"])


_VDT = {0: np.float64, 1: np.int32, 2: None}


class _Packed:
    """host arrays in one guarded device buffer, each at a 16-byte aligned place"""

    def __init__(self):
        self.parts, self.nbytes = [], 0

    def add(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        at = self.nbytes
        self.parts.append((at, a))
        self.nbytes += -(-max(a.nbytes, 1) // 16) * 16
        return at

    def upload(self):
        host = np.zeros(max(self.nbytes, 16), np.uint8)
        for at, a in self.parts:
            host[at:at + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.g = GuardedVec(np.uint8, data=host)
        return self.g.ptr.value


def _typed(kind, x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.float64 if kind in (0, 3) else np.int32)


def dev_rbind_batch(objs, out_kind):
    """mxd_csr_rbind_batch on guarded buffers: dict(indptr, indices, values)"""
    lib = _lib.load()
    pack, places = _Packed(), []
    for kind, p, j, x, nr in objs:
        places.append((None if p is None else pack.add(np.asarray(p, np.int32)), pack.add(np.asarray(j, np.int32)),
                       pack.add(_typed(kind, x))))
    base = pack.upload()
    items = (_lib.RbindItem * max(len(objs), 1))()
    row = pos = 0
    for k, ((kind, p, j, x, nr), (ap, aj, ax)) in enumerate(zip(objs, places)):
        n = int(np.asarray(j).size)
        items[k] = _lib.RbindItem(kind, 1 if kind >= 3 else int(nr), None if ap is None else base + ap,
                                  None if aj is None else base + aj, None if ax is None else base + ax, n, pos, row)
        row += 1 if kind >= 3 else int(nr)
        pos += n
    gt = GuardedVec(np.uint8, data=np.frombuffer(bytes(items), dtype=np.uint8)[:C.sizeof(_lib.RbindItem) * len(objs)])
    gp, gj = GuardedVec(np.int32, n=row + 1), GuardedVec(np.int32, n=pos + SLACK)
    gx = None if out_kind == 2 else GuardedVec(_VDT[out_kind], n=pos + SLACK)
    check(lib.mxd_csr_rbind_batch(gt.ptr if objs else None, len(objs), out_kind, row, pos, gp.ptr, gj.ptr,
                                  None if gx is None else gx.ptr, None))
    _sync()
    pack.g.assert_untouched()
    gt.assert_untouched()
    return dict(indptr=gp.result(), indices=gj.result(pos), values=None if gx is None else gx.result(pos))


def dev_coo_rbind(objs, out_kind):
    """mxd_coo_rbind_append, one call per operand (kind, i | None, j, values | None, nrows): dict(ii, jj, xx)"""
    lib = _lib.load()
    total = nnz_of(objs)
    gi, gj = GuardedVec(np.int32, n=total + SLACK), GuardedVec(np.int32, n=total + SLACK)
    gx = None if out_kind == 2 else GuardedVec(_VDT[out_kind], n=total + SLACK)
    row = pos = 0
    inputs = []
    for kind, i, j, x, nr in objs:
        ii = None if i is None else GuardedVec(np.int32, data=i)
        jj, xx = GuardedVec(np.int32, data=j), None if x is None else GuardedVec(_typed(kind, x).dtype, data=_typed(kind, x))
        inputs += [ii, jj, xx]
        check(lib.mxd_coo_rbind_append(kind, None if ii is None else ii.ptr, jj.ptr, None if xx is None else xx.ptr, jj.n,
                                       out_kind, row, pos, gi.ptr, gj.ptr, None if gx is None else gx.ptr, None))
        row += 1 if kind >= 3 else int(nr)
        pos += jj.n
    _sync()
    for g in inputs:
        if g is not None:
            g.assert_untouched()
    return dict(ii=gi.result(total), jj=gj.result(total), xx=None if gx is None else gx.result(total))


def dev_cbind_svec(X, ncol, x_kind, vi_sorted, vx, v_kind, length, first, out_kind):
    """mxd_csr_cbind_svec on guarded buffers (the vector's indices sorted): dict(indptr, indices, values)"""
    lib = _lib.load()
    kind, p, j, x, nX = X
    gp_in, gj_in = GuardedVec(np.int32, data=p), GuardedVec(np.int32, data=j)
    gx_in = None if x is None else GuardedVec(_typed(x_kind, x).dtype, data=_typed(x_kind, x))
    gvi = GuardedVec(np.int32, data=vi_sorted)
    gvx = None if vx is None else GuardedVec(_typed(v_kind, vx).dtype, data=_typed(v_kind, vx))
    nrows, nout = max(nX, length), int(np.asarray(j).size) + gvi.n
    gp, gj = GuardedVec(np.int32, n=nrows + 1), GuardedVec(np.int32, n=nout + SLACK)
    gx = None if out_kind == 2 else GuardedVec(_VDT[out_kind], n=nout + SLACK)
    check(lib.mxd_csr_cbind_svec(nX, ncol, gp_in.ptr, gj_in.ptr, None if gx_in is None else gx_in.ptr, x_kind, gvi.ptr,
                                 None if gvx is None else gvx.ptr, v_kind, gvi.n, length, int(first), out_kind, gp.ptr,
                                 gj.ptr, None if gx is None else gx.ptr, None))
    _sync()
    for g in (gp_in, gj_in, gx_in, gvi, gvx):
        if g is not None:
            g.assert_untouched()
    return dict(indptr=gp.result(), indices=gj.result(nout), values=None if gx is None else gx.result(nout))
