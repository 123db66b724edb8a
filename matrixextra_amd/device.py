"""Device-resident operands and mxd_* launches on torch tensors.

torch is plumbing here: it owns the HBM allocations, the stream and (in
distributed.py) the RCCL communicator; every kernel that runs is one of
libmxgpu.so's hand-written HIP kernels, launched on torch's current stream
through the device-level C-ABI (include/mxgpu.h, mxd_*).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import MX_F32, MX_F64, MX_LGL, MX_NONE, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@dataclass
class DeviceCSR:
    """CSR arrays resident in HBM: int32 indptr[m+1], int32 indices[nnz], values (f64 / int32 logical / None)."""
    indptr: torch.Tensor
    indices: torch.Tensor
    values: torch.Tensor | None
    m: int
    K: int
    nnz: int
    _sorted: bool | None = None
    _plan: object = None
    _plan_panels: int = -1
    _order: object = None
    _order_builds: int = 0
    _rows: object = None

    def plan(self, npanels: int = 0, rebuild: bool = False):
        """Device-resident SpMM plan (mxd_spmm_plan_create); cached per DeviceCSR, buffers re-used on rebuild."""
        lib = _lib.load()
        if self._plan is None or rebuild or self._plan_panels != npanels:
            handle = self._plan if self._plan is not None else C.c_void_p()
            check(lib.mxd_spmm_plan_create(self.m, self.K, _dp(self.indptr), _dp(self.indices), _dp(self.values),
                                           npanels, _stream(), C.byref(handle)))
            self._plan, self._plan_panels = handle, npanels
        return self._plan

    def plan_info(self):
        lib = _lib.load()
        P, padded = C.c_int(0), C.c_int64(0)
        check(lib.mxd_spmm_plan_info(self._plan, C.byref(P), C.byref(padded)))
        return dict(npanels=P.value, padded_entries=padded.value)

    def __del__(self):
        try:
            if self._plan is not None:
                _lib.load().mxd_spmm_plan_destroy(self._plan)
        except Exception:
            pass

    def rows_sorted(self) -> bool:
        """check_is_sorted per row on the device (src/misc.cpp:118-128); cached."""
        if self._sorted is None:
            ws = _int32(self.indptr.device, 4)
            flag, = _call("mxd_csr_rows_sorted", self.m, _dp(self.indptr), _dp(self.indices), _dp(ws), cells=(C.c_int,))
            self._sorted = bool(flag)
        return self._sorted

    def column_order(self):
        """(perm, colptr) of the pattern through mxd_csr_column_order: perm[q] is the row-major
        position of the q-th entry in column-major order, colptr the column pointer.  Cached beside the plan: it
        depends on indptr and indices only, so it also serves any DeviceCSR that shares them (col_reduce's `order`)."""
        if self._order is None:
            dev = self.indptr.device
            ws = _workspace(dev, "mxd_csr_transpose_workspace_bytes", self.nnz)
            perm, = _entries(dev, self.nnz, torch.int32)
            colptr = _int32(dev, self.K + 1)
            _call("mxd_csr_column_order", self.m, self.K, _dp(self.indptr), _dp(self.indices), self.nnz, _dp(perm),
                  _dp(colptr), _dp(ws))
            self._order = (perm[:self.nnz], colptr)
            self._order_builds += 1
        return self._order

    def entry_rows(self, order=None):
        """The row of every entry in column order (mxd_csr_transpose_by_order without values): with
        the colptr of the order the pattern of X^T.  Cached beside the order, which it goes through: column_order(),
        or `order`, the (perm, colptr) of a DeviceCSR that shares indptr and indices."""
        if self._rows is None:
            perm, _ = _order_of("entry_rows", self, order)
            rows, = _entries(self.indptr.device, self.nnz, torch.int32)
            _call("mxd_csr_transpose_by_order", self.m, self.nnz, _dp(self.indptr), None, MX_NONE, _dp(perm), _dp(rows),
                  None)
            self._rows = rows[:self.nnz]
        return self._rows

    def transposed(self, order=None):
        """X^T (K x m) as a DeviceCSR: indptr is the cached colptr, indices the cached entry rows, and the values are
        gathered through the order now (None stays None), so a matrix whose values changed pays one gather and no
        sort.  Its rows are sorted: the order is stable.  order: as col_reduce takes it."""
        perm, colptr = _order_of("transposed", self, order)
        rows = self.entry_rows(order)
        values = None
        if self.values is not None:
            values, = _entries(self.indptr.device, self.nnz, self.values.dtype)
            _call("mxd_csr_transpose_by_order", self.m, self.nnz, _dp(self.indptr), _dp(self.values),
                  _value_dtype(self.values), _dp(perm), None, _dp(values))
            values = values[:self.nnz]
        return DeviceCSR(colptr, rows, values, self.K, self.m, self.nnz, _sorted=True)

    @classmethod
    def from_host(cls, indptr, indices, values, K, device="cuda"):
        p = torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int32)).to(device)
        j = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(device)
        x = None if values is None else torch.from_numpy(np.ascontiguousarray(values)).to(device)
        return cls(p, j, x, int(p.numel() - 1), int(K), int(j.numel()))

    def to_host(self):
        return (self.indptr.cpu().numpy(), self.indices.cpu().numpy(),
                None if self.values is None else self.values.cpu().numpy())


def _spmm_out(A: DeviceCSR, B: torch.Tensor, out: torch.Tensor | None, colmajor: bool):
    """Checks B and `out` of an SpMM launch (the kernels write m x n elements at ldc = n, or n x m at ldc = m, and
    nothing checks that on the device side); allocates `out` when it is None.  Returns (out, ldc)."""
    if B.dim() != 2 or B.stride(1) != 1 or B.shape[0] != A.K or B.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"B must be a {A.K} x n float64 / float32 tensor with unit column stride, "
                         f"got {tuple(B.shape)} {B.dtype} with strides {B.stride()}")
    n = int(B.shape[1])
    shape = (n, A.m) if colmajor else (A.m, n)
    if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != B.dtype
                            or out.device != B.device):
        raise ValueError(f"out must be a contiguous {shape} {B.dtype} tensor on {B.device}, "
                         f"got {tuple(out.shape)} {out.dtype} on {out.device} (contiguous: {out.is_contiguous()})")
    if not B.is_cuda:
        raise ValueError("B must be a device tensor")
    if out is None:
        out = torch.empty(shape, dtype=B.dtype, device=B.device)
    return out, shape[1]


def spmm(A: DeviceCSR, B: torch.Tensor, out: torch.Tensor | None = None, colmajor: bool = False,
         algo: int = 0, npanels: int = 0, wg_per_cu: int = 0):
    """C = A @ B with B (K x n) row-major in HBM.  colmajor=False: C row-major (m x n) —
    gemm_csr_drm_as_drm layout; colmajor=True: C column-major (what tcrossprod_csr_dense returns to R),
    stored as a row-major (n x m) tensor and returned as its transposed view.
    algo: 0 auto, 1 row-wave kernel, 2 slab/panel kernel (include/mxgpu.h mx_spmm_algo)."""
    out, ldc = _spmm_out(A, B, out, colmajor)
    lib = _lib.load()
    n = int(B.shape[1])
    dt = MX_F64 if B.dtype == torch.float64 else MX_F32
    if A.nnz == 0:                       # reference early-out (matmul.cpp:128-129,160-161): all zeros
        out.zero_()
        return out.t() if colmajor else out
    sorted_rows = A.rows_sorted() if algo != 1 else False
    check(lib.mxd_spmm_csr_dense_ex(A.m, n, A.K, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(B), B.stride(0),
                                    _dp(out), ldc, dt, 1 if colmajor else 0, algo, int(sorted_rows), npanels, wg_per_cu,
                                    _stream()))
    return out.t() if colmajor else out


def spmm_planned(A: DeviceCSR, B: torch.Tensor, out: torch.Tensor | None = None, colmajor: bool = False,
                 npanels: int = 0, wg_per_cu: int = 0, sync_mode: int = -1, rebuild_plan: bool = False):
    """C = A @ B through the planned panel-sweep kernel (v3).  The plan is built on first use (or every call with
    rebuild_plan=True, which is what a one-shot product from plain CSR costs) and cached on the DeviceCSR."""
    out, ldc = _spmm_out(A, B, out, colmajor)
    lib = _lib.load()
    n = int(B.shape[1])
    dt = MX_F64 if B.dtype == torch.float64 else MX_F32
    if A.nnz == 0:
        out.zero_()
        return out.t() if colmajor else out
    plan = A.plan(npanels, rebuild=rebuild_plan)
    check(lib.mxd_spmm_plan_run(plan, n, _dp(B), B.stride(0), _dp(out), ldc, dt, 1 if colmajor else 0, wg_per_cu,
                                sync_mode, _stream()))
    return out.t() if colmajor else out


def spmv(A: DeviceCSR, v: torch.Tensor, v_dtype=None, out=None):
    """y = A @ v (matmul_csr_dvec).  v float64 / float32 / int32 (v_dtype MX_I32 or MX_LGL for int32)."""
    lib = _lib.load()
    if v_dtype is None:
        v_dtype = {torch.float64: MX_F64, torch.float32: MX_F32}[v.dtype]
    odt = torch.float32 if v_dtype == MX_F32 else torch.float64
    if out is None:
        out = torch.empty(A.m, dtype=odt, device=v.device)
    check(lib.mxd_spmv_csr_dvec(A.m, A.nnz, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(v), v_dtype, _dp(out),
                                _stream()))
    return out


# ---- what the wrappers below are made of: kinds, buffers, the call, operand checks, the second pass --
def _value_dtype(values) -> int:
    """The mx_dtype of a values tensor; the only place that maps one."""
    if values is None:
        return MX_NONE
    if values.dtype == torch.float64:
        return MX_F64
    if values.dtype == torch.int32:
        return MX_LGL
    raise ValueError(f"values must be float64 or int32 (R logical), got {values.dtype}")


def _dtype(values):
    return None if values is None else values.dtype


def _float_dtype(t) -> int:
    """MX_F64 / MX_F32 of a dense float operand"""
    return MX_F64 if t.dtype == torch.float64 else MX_F32


# dense_kind of the products with a dense operand (mxgpu.h): 0 double, 1 float32, 2 R integer, 3 R logical
_DENSE_DOUBLE, _DENSE_FLOAT32, _DENSE_INTEGER, _DENSE_LOGICAL = range(4)
# mx_rbind_input.kind (mxgpu.h): 0 dgR, 1 lgR, 2 ngR, 3 dsparseVector, 4 isparseVector, 5 lsparseVector, 6 nsparseVector
_DGR, _LGR, _NGR, _DSVEC, _ISVEC, _LSVEC, _NSVEC = range(7)


def _dense_kind(what: str, X: torch.Tensor, logical: bool):
    """(X as the kernels read it, its dense_kind): bool becomes int32 R logicals, int32 is R integer, or R logical
    with `logical`."""
    if X.dtype == torch.bool:
        return X.to(torch.int32), _DENSE_LOGICAL
    if X.dtype == torch.int32:
        return X, _DENSE_LOGICAL if logical else _DENSE_INTEGER
    if X.dtype == torch.float64:
        return X, _DENSE_DOUBLE
    if X.dtype == torch.float32:
        return X, _DENSE_FLOAT32
    raise ValueError(f"{what}: unsupported dense dtype {X.dtype}")


def _scratch(dev, nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _workspace(dev, size_fn: str, *args):
    """The workspace of one kernel family: as many bytes as its mxd_*_workspace_bytes(*args) asks for."""
    return _scratch(dev, getattr(_lib.load(), size_fn)(*args))


def _int32(dev, n):
    return torch.empty(n, dtype=torch.int32, device=dev)


def _entries(dev, k, *dtypes, floor=1):
    """One buffer of k elements per dtype, None (no values) giving None.  A buffer is never shorter than `floor`:
    most kernels are handed a valid pointer for an empty result too; floor=0 allocates exactly k."""
    return [None if dt is None else torch.empty(max(k, floor), dtype=dt, device=dev) for dt in dtypes]


_COUNT = (C.c_int64,)       # the host cell of a count pass


def _call(fn: str, *args, cells=()):
    """check(lib.<fn>(*args, one host out-cell per ctypes type in `cells`, the stream)): in every mxd_* prototype the
    *_host parameters stand directly in front of the stream.  Returns the cells' values as plain Python numbers."""
    cells = [t() for t in cells]
    check(getattr(_lib.load(), fn)(*args, *map(C.byref, cells), _stream()))
    return [c.value for c in cells]


def _fill_pass(dev, k, dtypes, fill, floor=1, always=False):
    """The second half of a count -> fill family, given the count k that the first pass read back: one entry buffer
    per dtype (_entries), `fill(*buffers)`, the buffers cut to k entries.  An empty result launches no fill, unless
    `always`: csr_elemwise, csr_gather_rows, _csr_compact and csc_by_dense launch theirs (every fill accepts an empty
    result; skipping it only saves a launch).  The count pass is a plain _call in front, so what else it reads back,
    and any decision between the passes, stays a local variable of the wrapper."""
    buffers = _entries(dev, k, *dtypes, floor=floor)
    if k or always:
        fill(*buffers)
    if k >= floor:              # the buffers are k long already
        return buffers
    return [b if b is None else b[:k] for b in buffers]


def _coo_triplets(i, j, x, need_x=False, int32=True) -> int:
    """nnz of the COO triplets (i, j, x), checked: equal lengths (x may be None unless need_x) and, with int32,
    contiguous int32 i and j."""
    nnz = int(i.numel())
    if int(j.numel()) != nnz or (x is None and need_x) or (x is not None and int(x.numel()) != nnz):
        raise ValueError("i, j and x must have the same length")
    if int32 and (i.dtype != torch.int32 or j.dtype != torch.int32 or not (i.is_contiguous() and j.is_contiguous())):
        raise ValueError("i and j must be contiguous int32 tensors")
    return nnz


def _svec(what: str, dev, vi, vx, vx_dtypes=(torch.float64,), pattern=True):
    """The sparse vector (vi, vx) of a product, checked and contiguous: vi 1-d int32 on dev; vx of one of vx_dtypes,
    of vi's shape and on dev, or, where the product takes an nsparseVector (`pattern`), None."""
    if vi.dtype != torch.int32 or vi.dim() != 1 or vi.device != dev:
        raise ValueError(f"{what}: vi must be a 1-d int32 tensor on {dev}")
    if not (pattern and vx is None) and (vx.dtype not in vx_dtypes or vx.shape != vi.shape or vx.device != dev):
        names = " or ".join(str(dt).replace("torch.", "") for dt in vx_dtypes)
        raise ValueError(f"{what}: vx must be {names}, of vi's shape and on its device")
    return vi.contiguous(), None if vx is None else vx.contiguous()


def _bind_indices(message: str, j, x):
    """An operand of a bind is read in place: contiguous int32 indices, and values, where there are any, as many."""
    if j.dtype != torch.int32 or not j.is_contiguous() or (x is not None and int(x.numel()) != int(j.numel())):
        raise ValueError(message)


def _order_of(what: str, A: DeviceCSR, order):
    """(perm, colptr) for A: its own cached column order, or the caller's, checked against A's sizes"""
    perm, colptr = A.column_order() if order is None else order
    if int(colptr.numel()) != A.K + 1 or int(perm.numel()) != A.nnz:
        raise ValueError(f"{what}: the order belongs to another pattern")
    return perm, colptr


def _f64_values(what: str, A: DeviceCSR):
    if A.values is None or A.values.dtype != torch.float64:
        raise ValueError(f"{what}: X needs float64 values")


def csr_elemwise(op, A: DeviceCSR, B: DeviceCSR):
    """CSR (+) CSR on device-resident operands: count -> scan -> (one host round trip for nnz) -> fill."""
    assert A.m == B.m
    dev = A.indptr.device
    ws = _workspace(dev, "mxd_merge_workspace_bytes", A.m)
    out_p = _int32(dev, A.m + 1)
    k, = _call("mxd_csr_merge_count", op, A.m, _dp(A.indptr), _dp(A.indices), A.nnz, _dp(B.indptr), _dp(B.indices),
               B.nnz, _dp(out_p), _dp(ws), cells=_COUNT)
    logical = op in (_lib.MX_OP_OR, _lib.MX_OP_XOR, _lib.MX_OP_AND)
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, torch.int32 if logical else torch.float64),
        lambda oj, ox: _call("mxd_csr_merge_fill", op, A.m, _dp(A.indptr), _dp(A.indices), _dp(A.values), A.nnz,
                             _dp(B.indptr), _dp(B.indices), _dp(B.values), B.nnz, _dp(out_p), _dp(oj), _dp(ox)),
        floor=0, always=True)
    return DeviceCSR(out_p, out_j, out_x, A.m, A.K, k)


def csr_gather_rows(A: DeviceCSR, rows: torch.Tensor):
    """A[rows, :] on device (copy_csr_rows).  rows int32, 0-based."""
    dev = A.indptr.device
    vd = _value_dtype(A.values)
    r = int(rows.numel())
    ws = _workspace(dev, "mxd_gather_workspace_bytes", r)
    new_p = _int32(dev, r + 1)
    k, = _call("mxd_csr_gather_count", r, _dp(A.indptr), _dp(rows), _dp(new_p), _dp(ws), cells=_COUNT)
    new_j, new_x = _fill_pass(
        dev, k, (torch.int32, _dtype(A.values)),
        lambda nj, nx: _call("mxd_csr_gather_fill", r, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(rows),
                             _dp(new_p), _dp(nj), _dp(nx), vd, k),
        floor=0, always=True)
    return DeviceCSR(new_p, new_j, new_x, r, A.K, k)


def csr_transpose(A: DeviceCSR) -> DeviceCSR:
    """CSR of A^T (equivalently: CSR <-> CSC) on device-resident operands through mxd_csr_transpose: rows of the
    result in ascending source-row order, values copied bit for bit, repeated (row, col) pairs merged."""
    dev = A.indptr.device
    vd = _value_dtype(A.values)
    ws = _workspace(dev, "mxd_csr_transpose_workspace_bytes", A.nnz)
    out_p = _int32(dev, A.K + 1)
    out_j, out_x = _entries(dev, A.nnz, torch.int32, _dtype(A.values))
    nnz, = _call("mxd_csr_transpose", A.m, A.K, _dp(A.indptr), _dp(A.indices), _dp(A.values), vd, A.nnz, _dp(out_p),
                 _dp(out_j), _dp(out_x), _dp(ws), cells=_COUNT)
    return DeviceCSR(out_p, out_j[:nnz], None if out_x is None else out_x[:nnz], A.K, A.m, nnz)


def coo_to_csr(i: torch.Tensor, j: torch.Tensor, x: torch.Tensor | None, m: int, n: int) -> DeviceCSR:
    """Canonical CSR of an m x n COO held in HBM (int32 0-based triplets, any order) through mxd_coo_to_csr:
    columns ascending and unique per row, repeated (i, j) merged by Matrix's triplet rules.  coo_to_csr(j, i, x,
    n, m) gives the CSC arrays."""
    dev = i.device
    nnz = _coo_triplets(i, j, x)
    vd = _value_dtype(x)
    ws = _workspace(dev, "mxd_coo_to_csr_workspace_bytes", nnz, int(n))
    out_p = _int32(dev, int(m) + 1)
    out_j, out_x = _entries(dev, nnz, torch.int32, _dtype(x))
    k, = _call("mxd_coo_to_csr", int(m), int(n), _dp(i), _dp(j), _dp(x), vd, nnz, _dp(out_p), _dp(out_j), _dp(out_x),
               _dp(ws), cells=_COUNT)
    return DeviceCSR(out_p, out_j[:k], None if out_x is None else out_x[:k], int(m), int(n), k)


def csr_to_coo(A: DeviceCSR):
    """(i, j, x) of a device CSR in storage order through mxd_csr_to_coo: i is new, j and x are A's own tensors."""
    rows, = _entries(A.indptr.device, A.nnz, torch.int32)
    _call("mxd_csr_to_coo", A.m, A.nnz, _dp(A.indptr), _dp(rows))
    return rows[:A.nnz], A.indices, A.values


def coo_sort(i: torch.Tensor, j: torch.Tensor, x: torch.Tensor | None, byrow: bool = True) -> bool:
    """Sorts COO triplets held in HBM (int32 0-based, non-negative) in place through mxd_coo_sort: by (i, j), or by
    (j, i) with byrow=False; x (f64, int32 R logicals, or None) follows.  Entries of one cell keep their input order.
    Returns whether the triplets were already sorted, in which case nothing was written."""
    nnz = _coo_triplets(i, j, x)
    if x is not None and not x.is_contiguous():
        raise ValueError("x must be a contiguous tensor")
    vd = _value_dtype(x)
    ws = _workspace(i.device, "mxd_coo_sort_workspace_bytes", nnz)
    first, second = (i, j) if byrow else (j, i)
    was_sorted, = _call("mxd_coo_sort", _dp(first), _dp(second), _dp(x), nnz, vd, _dp(ws), cells=(C.c_int,))
    return bool(was_sorted)


CooAxis = _lib.CooAxis      # mx_coo_axis, as include/mxgpu.h declares it


def _coo_axis(take_base1: torch.Tensor | None, kind: str, n: int, lo: int = 0, hi: int = -1):
    """(mx_coo_axis, tensors it points to) for one axis of coo_slice."""
    if kind == "all":
        return CooAxis(0, 0, n - 1, 0, 0, None, None), ()
    if kind in ("seq", "rev"):
        return CooAxis(0, int(lo), int(hi), int(kind == "rev"), 0, None, None), ()
    dev = take_base1.device
    nt = int(take_base1.numel())
    nmap = int(take_base1.max().item()) + 1 if nt else 1
    start = _int32(dev, nmap + 1)
    pos, = _entries(dev, nt, torch.int32)
    ws = _workspace(dev, "mxd_colmap_workspace_bytes", nmap)
    _call("mxd_colmap_build", _dp(take_base1), nt, nmap, _dp(start), _dp(pos), _dp(ws))
    return CooAxis(1, 0, 0, 0, nmap, start.data_ptr(), pos.data_ptr()), (start, pos, ws)


def coo_slice(i: torch.Tensor, j: torch.Tensor, x: torch.Tensor | None, m: int, n: int, rows, cols):
    """X[rows, cols] of an m x n COO held in HBM through mxd_coo_slice_count / _fill, as (i, j, x) of the result.
    Each selector is ("all",), ("seq", lo, hi) / ("rev", lo, hi) with 0-based bounds (positions r - lo / hi - r),
    or ("map", take_base1) with a 1-based int32 tensor (any order, repeats allowed)."""
    dev = i.device
    nnz = _coo_triplets(i, j, x, int32=False)
    vd = _value_dtype(x)

    def axis(sel, size):
        if sel[0] == "map":
            return _coo_axis(sel[1], "map", size)
        if sel[0] == "all":
            return _coo_axis(None, "all", size)
        return _coo_axis(None, sel[0], size, sel[1], sel[2])

    ai, keep_i = axis(rows, m)
    aj, keep_j = axis(cols, n)
    ws = _workspace(dev, "mxd_coo_slice_workspace_bytes", nnz)
    k, = _call("mxd_coo_slice_count", int(m), int(n), _dp(i), _dp(j), nnz, C.byref(ai), C.byref(aj), _dp(ws),
               cells=_COUNT)
    out = _fill_pass(
        dev, k, (torch.int32, torch.int32, _dtype(x)),
        lambda oi, oj, ox: _call("mxd_coo_slice_fill", int(m), int(n), _dp(i), _dp(j), _dp(x), vd, nnz, C.byref(ai),
                                 C.byref(aj), _dp(ws), _dp(oi), _dp(oj), _dp(ox)))
    del keep_i, keep_j          # the maps stay alive until both launches are enqueued (torch's caching allocator
    return tuple(out)           # reuses the blocks only on this same stream)


def coo_inject_na(i: torch.Tensor, j: torch.Tensor, x: torch.Tensor, m: int, n: int, rows_na: torch.Tensor,
                  cols_na: torch.Tensor):
    """NA rows / columns injected into an m x n COO held in HBM through mxd_coo_inject_na_count / _fill (DESIGN.md
    §4.18), as (i, j, x) of the result: the triplets that stay, in storage order, then the NA block.  x: float64
    (NA_real_) or int32 R logicals (NA_LOGICAL); rows_na / cols_na: int32 tensors of 0-based indices, ascending and
    distinct (either may be empty)."""
    dev = i.device
    nnz = _coo_triplets(i, j, x, need_x=True, int32=False)
    for t in (i, j, rows_na, cols_na):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"i, j, rows_na and cols_na must be contiguous int32 tensors on {dev}")
    vd = _value_dtype(x)
    n_rna, n_cna = int(rows_na.numel()), int(cols_na.numel())
    ws = _workspace(dev, "mxd_compact_workspace_bytes", nnz)
    maps = _int32(dev, 4 + int(m) + int(n) + max(int(m), int(n)))
    k, = _call("mxd_coo_inject_na_count", int(m), int(n), _dp(i), _dp(j), nnz, _dp(rows_na), n_rna, _dp(cols_na),
               n_cna, _dp(ws), _dp(maps), cells=_COUNT)
    return tuple(_fill_pass(
        dev, k, (torch.int32, torch.int32, x.dtype),
        lambda oi, oj, ox: _call("mxd_coo_inject_na_fill", int(m), int(n), _dp(i), _dp(j), _dp(x.contiguous()), vd,
                                 nnz, _dp(rows_na), n_rna, _dp(cols_na), n_cna, _dp(ws), _dp(maps), _dp(oi), _dp(oj),
                                 _dp(ox))))


def csr_single(A: DeviceCSR, r: int, c: int):
    """A[r, c] (0-based) of a device-resident CSR through mxd_csr_single: (found, value) of the first entry of row r,
    in storage order, at column c; value is None for a pattern matrix or a miss."""
    if not 0 <= int(r) < A.m:
        raise ValueError(f"csr_single: row {r} outside [0, {A.m})")
    vd = _value_dtype(A.values)
    ws = _scratch(A.indptr.device, 16)
    k, val = _call("mxd_csr_single", A.m, _dp(A.indptr), _dp(A.indices), _dp(A.values), vd, A.nnz, int(r), int(c),
                   _dp(ws), cells=(C.c_int64, C.c_double if vd == MX_F64 else C.c_int32))
    if k < 0:
        return False, None
    return True, (None if vd == MX_NONE else val)


def _csr_compact(A: DeviceCSR, rule: int, mask: torch.Tensor | None) -> DeviceCSR:
    """count (one 8-byte read-back) -> fill through mxd_compact_count / _fill; A itself when a zero rule keeps all."""
    dev = A.indptr.device
    vd = _value_dtype(A.values)
    ws = _workspace(dev, "mxd_compact_workspace_bytes", A.nnz)
    k, = _call("mxd_compact_count", A.nnz, _dp(A.values), vd, rule, _dp(mask), _dp(ws), cells=_COUNT)
    if k == A.nnz and rule != _lib.MX_KEEP_MASK:
        return A
    out_p = _int32(dev, A.m + 1)
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, A.values.dtype),
        lambda oj, ox: _call("mxd_compact_fill", A.nnz, _dp(A.values), vd, rule, _dp(mask), _dp(A.indices), None, A.m,
                             _dp(A.indptr), _dp(ws), _dp(oj), None, _dp(ox), _dp(out_p)),
        always=True)
    return DeviceCSR(out_p, out_j, out_x, A.m, A.K, k)


def csr_remove_zeros(A: DeviceCSR, na_rm: bool = False) -> DeviceCSR:
    """remove_sparse_zeros of a device-resident CSR (or CSC) with the reference's keep rules (remove_zero_valued_csr_*,
    src/misc.cpp:553-699): f64 drops 0 (and NaN with na_rm); R logicals drop FALSE, or with na_rm only NA.  Returns
    A itself when nothing is removed (and for a pattern A)."""
    if A.values is None:
        return A
    vd = _value_dtype(A.values)
    rule = _lib.MX_KEEP_NONZERO
    if na_rm:
        rule = _lib.MX_KEEP_NONZERO_NOT_NA if vd == MX_F64 else _lib.MX_KEEP_NOT_NA
    return _csr_compact(A, rule, None)


def csc_by_dense(A: DeviceCSR, D: torch.Tensor, keep_na: bool = True, logical: bool = False):
    """X * D for a device-resident CSC X and a dense tensor D of X's shape, as (p, i, x) tensors.
    A holds X's CSC arrays as the CSR of X^T: A.indptr over the A.m columns, A.indices the rows, f64 A.values,
    A.K = rows.  D: float64, float32, int32 (R integer; R logical with logical=True) or bool (R logical), any strides.
    keep_na=True: every NA cell of D outside X's pattern becomes an NA_real_ entry and a repeated row is kept once
    (rows must be sorted inside each column); the result is new tensors.  keep_na=False: values only; the result is
    A.indptr itself, a copy of A.indices and the new values."""
    dev = A.indptr.device
    _f64_values("csc_by_dense", A)
    if D.dim() != 2 or tuple(D.shape) != (A.K, A.m):
        raise ValueError(f"csc_by_dense: D must be {A.K} x {A.m}")
    D, kind = _dense_kind("csc_by_dense", D, logical)
    Dc = D.t().contiguous()                         # row-major D^T = column-major D
    out_x, = _entries(dev, A.nnz, torch.float64)

    def values_only():
        _call("mxd_csc_by_dense_elemwise", A.m, A.K, A.nnz, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(Dc), kind,
              _dp(out_x))
        return out_x[:A.nnz]

    if not keep_na:
        return A.indptr, A.indices.clone(), values_only()
    ws = _workspace(dev, "mxd_csc_dense_na_workspace_bytes", A.K, A.m)
    k, outside = _call("mxd_csc_dense_na_count", A.K, A.m, A.nnz, _dp(A.indptr), _dp(A.indices), _dp(Dc), kind, _dp(ws),
                       cells=_COUNT * 2)
    if outside == 0 and k == A.nnz:                 # the structure does not change: values only, new p and i
        return A.indptr.clone(), A.indices.clone(), values_only()
    out_p = _int32(dev, A.m + 1)
    out_i, out_x = _fill_pass(
        dev, k, (torch.int32, torch.float64),
        lambda oi, ox: _call("mxd_csc_dense_na_fill", A.K, A.m, A.nnz, _dp(A.indptr), _dp(A.indices), _dp(A.values),
                             _dp(Dc), kind, _dp(ws), _dp(out_p), _dp(oi), _dp(ox)),
        always=True)
    return out_p, out_i, out_x


def csr_by_svec(A: DeviceCSR, vi: torch.Tensor, vx: torch.Tensor | None, length: int, keep_na: bool = True):
    """X * v for a device-resident CSR X (f64 values, sorted rows) and a sparse vector recycled down its rows
    (DESIGN.md §4.11), as (p, j, x) tensors.  vi: sorted 1-based int32 positions; vx: their f64 values, or None for
    an nsparseVector; length must divide A.m.  Rows whose position v does not store drop out, the others are scaled.
    keep_na=True also keeps the NaN / Inf entries of dropped rows (as NaN) and fills every column of a row whose
    vector value is NaN / Inf."""
    dev = A.indptr.device
    _f64_values("csr_by_svec", A)
    vi, vx = _svec("csr_by_svec", dev, vi, vx)
    length, nv, keep = int(length), int(vi.numel()), int(bool(keep_na))
    if A.m and (length <= 0 or length > A.m or A.m % length or nv > length):
        raise ValueError("csr_by_svec: the vector's length must divide the number of rows")
    ws = _workspace(dev, "mxd_csr_by_svec_workspace_bytes", A.m)
    out_p = _int32(dev, A.m + 1)
    k, _ = _call("mxd_csr_by_svec_count", A.m, A.K, A.nnz, _dp(A.indptr), _dp(A.values), _dp(vi), nv, _dp(vx), length,
                 keep, _dp(ws), _dp(out_p), cells=_COUNT * 2)
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, torch.float64),
        lambda oj, ox: _call("mxd_csr_by_svec_fill", A.m, A.K, A.nnz, _dp(A.indptr), _dp(A.indices), _dp(A.values),
                             _dp(vi), nv, _dp(vx), length, keep, _dp(ws), _dp(out_p), _dp(oj), _dp(ox)))
    return out_p, out_j, out_x


def dense_by_svec(X: torch.Tensor, vi: torch.Tensor, vx: torch.Tensor, length: int, keep_na: bool = True,
                  logical: bool = False):
    """X * v for a device-resident dense matrix X and a sparse vector.  X: 2-d float64, float32,
    int32 (R integer; R logical with logical=True) or bool, any strides; vi: 1-based int32 positions inside
    1..length (sorted when keep_na is set); vx: their f64 values.  A length equal to the number of cells, or one that
    does not divide the number of rows, gives a float64 tensor of X's shape (column-major storage, the vector
    recycled over the cells); a length that divides the number of rows gives the CSR (p, j, x) of full rows.
    keep_na=True keeps the NA / NaN / Inf cells that the vector does not cover, as NA / NaN."""
    dev = X.device
    if X.dim() != 2:
        raise ValueError("dense_by_svec: X must be a matrix")
    X, kind = _dense_kind("dense_by_svec", X, logical)
    vi, vx = _svec("dense_by_svec", dev, vi, vx, pattern=False)
    nrows, ncols = int(X.shape[0]), int(X.shape[1])
    length, nv, keep = int(length), int(vi.numel()), int(bool(keep_na))
    route = _lib.load().mx_dense_by_svec_route(nrows, ncols, length)
    if route < 0:
        check(1)
    if nv > length:
        raise ValueError("dense_by_svec: the vector stores more positions than its length")
    if nv and (int(vi.min()) < 1 or int(vi.max()) > length):
        raise ValueError(f"dense_by_svec: positions must lie inside 1..{length}")
    Xc = X.t().contiguous()                         # row-major X^T = column-major X
    if route in (_lib.MX_DSV_ROUTE_A, _lib.MX_DSV_ROUTE_D):
        ws = _workspace(dev, "mxd_dense_by_svec_workspace_bytes", 0, length)
        out = torch.empty((ncols, nrows), dtype=torch.float64, device=dev)
        _call("mxd_dense_by_svec_dense", nrows, ncols, _dp(Xc), kind, _dp(vi), nv, _dp(vx), length, keep, _dp(ws),
              _dp(out))
        return out.t()
    ws = _workspace(dev, "mxd_dense_by_svec_workspace_bytes", nrows, length)
    out_p = _int32(dev, nrows + 1)
    k, = _call("mxd_dense_by_svec_count", nrows, ncols, _dp(Xc), kind, _dp(vi), nv, length, keep, _dp(ws), _dp(out_p),
               cells=_COUNT)
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, torch.float64),
        lambda oj, ox: _call("mxd_dense_by_svec_fill", nrows, ncols, _dp(Xc), kind, _dp(vx), length, keep, _dp(ws),
                             _dp(out_p), _dp(oj), _dp(ox)))
    return out_p, out_j, out_x


def csr_by_dvec_keep_na(A: DeviceCSR, v: torch.Tensor, op: str = "*"):
    """X op v (op one of * ^ / %% %/%) for a device-resident CSR X (f64 values, sorted rows) and a dense f64 vector
    recycled over the matrix, keeping the cells that R makes NA / NaN / 1 / Inf outside X's pattern,
    as (p, j, x) tensors.  A length that divides A.m rules whole rows; any other length up to A.m * A.K goes over the
    flat cells, and when that adds no entry the result's p and j are A's own tensors."""
    dev = A.indptr.device
    if op not in _lib.MX_DV_OPS:
        raise ValueError(f"csr_by_dvec_keep_na: unknown operation {op!r}")
    _f64_values("csr_by_dvec_keep_na", A)
    if v.dtype != torch.float64 or v.dim() != 1 or v.device != dev:
        raise ValueError(f"csr_by_dvec_keep_na: v must be a 1-d float64 tensor on {dev}")
    v = v.contiguous()
    L, code = int(v.numel()), _lib.MX_DV_OPS[op]
    m, K, nnz = A.m, A.K, A.nnz
    if L < 1 or (A.m % L and L > A.m * A.K):
        raise ValueError("csr_by_dvec_keep_na: v needs between 1 and nrow * ncol entries")
    out_p = _int32(dev, m + 1)
    if L <= A.m and A.m % L == 0:                                       # row-ruled
        ws = _workspace(dev, "mxd_csr_by_dvec_na_rows_workspace_bytes", m)
        k, = _call("mxd_csr_by_dvec_na_rows_count", m, K, nnz, _dp(A.indptr), _dp(v), L, code, _dp(ws), _dp(out_p),
                   cells=_COUNT)
        out_j, out_x = _fill_pass(
            dev, k, (torch.int32, torch.float64),
            lambda oj, ox: _call("mxd_csr_by_dvec_na_rows_fill", m, K, nnz, _dp(A.indptr), _dp(A.indices),
                                 _dp(A.values), _dp(v), L, code, _dp(out_p), _dp(oj), _dp(ox)))
        return out_p, out_j, out_x
    sws = _workspace(dev, "mxd_dvec_na_special_workspace_bytes", L)
    nsp, cand = _call("mxd_dvec_na_special", m, K, _dp(v), L, code, _dp(sws), cells=_COUNT * 2)
    n_new = 0
    if cand:
        cws = _workspace(dev, "mxd_dvec_na_cells_workspace_bytes", cand)
        n_new, = _call("mxd_dvec_na_cells_count", m, K, nnz, _dp(A.indptr), _dp(A.indices), L, _dp(sws), nsp, cand,
                       _dp(cws), cells=_COUNT)
    _, ax = _entries(dev, nnz, torch.int32, torch.float64)      # the int32 half is never used; the trace fixture pins it
    _call("mxd_csr_by_dvec", m, K, nnz, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(v), L, code, 1, _dp(ax))
    if n_new == 0:
        return A.indptr, A.indices, ax[:nnz]
    ni, nx, nj = _fill_pass(
        dev, n_new, (torch.int32, torch.float64, torch.int32),
        lambda i, x, j: _call("mxd_dvec_na_cells_fill", m, K, _dp(v), L, code, _dp(sws), nsp, cand, _dp(cws), _dp(i),
                              _dp(j), _dp(x)))
    B = coo_to_csr(ni, nj, nx, m, K)
    out_j, out_x = _fill_pass(
        dev, nnz + n_new, (torch.int32, torch.float64),
        lambda oj, ox: _call("mxd_csr_join_disjoint", m, _dp(A.indptr), _dp(A.indices), _dp(ax), nnz, _dp(B.indptr),
                             _dp(B.indices), _dp(B.values), n_new, _dp(out_p), _dp(oj), _dp(ox)))
    return out_p, out_j, out_x


def csr_filter(A: DeviceCSR, mask: torch.Tensor) -> DeviceCSR:
    """filterSparse of a device-resident CSR: keeps entry k where mask[k] (bool, or int32 R logical) is TRUE or NA;
    an NA writes NA_real_ / NA_LOGICAL as the value."""
    if A.values is None:
        raise ValueError("Method is only applicable for sparse objects with values (slot 'x').")
    if mask.dtype == torch.bool:
        mask = mask.to(torch.int32)
    if mask.dtype != torch.int32 or mask.numel() != A.nnz or mask.device != A.indptr.device:
        raise ValueError(f"mask must be {A.nnz} bool / int32 entries on {A.indptr.device}")
    return _csr_compact(A, _lib.MX_KEEP_MASK, mask.contiguous())


def _one_column(A: DeviceCSR, what: str):
    if A.K != 1:
        raise ValueError(f"{what}: X must have one column")
    _f64_values(what, A)


def csr_outer_dense(A: DeviceCSR, v: torch.Tensor):
    """X %*% v for a device-resident one-column CSR X (f64 values) and a dense f64 or f32 vector, as
    the (p, j, x) tensors of a CSR with A.m rows and v.numel() columns: every non-empty row of X times v, through the
    row's first stored value.  An f32 v gives the float product, widened."""
    dev = A.indptr.device
    _one_column(A, "csr_outer_dense")
    if v.dtype not in (torch.float64, torch.float32) or v.dim() != 1 or v.device != dev:
        raise ValueError(f"csr_outer_dense: v must be a 1-d float64 or float32 tensor on {dev}")
    v = v.contiguous()
    dim = int(v.numel())
    ws = _workspace(dev, "mxd_csr_outer_dense_workspace_bytes", A.m)
    out_p = _int32(dev, A.m + 1)
    k, = _call("mxd_csr_outer_dense_count", A.m, dim, _dp(A.indptr), _dp(ws), _dp(out_p), cells=_COUNT)
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, torch.float64),
        lambda oj, ox: _call("mxd_csr_outer_dense_fill", A.m, dim, A.nnz, _dp(A.indptr), _dp(A.values), _dp(v),
                             _float_dtype(v), _dp(out_p), _dp(oj), _dp(ox)))
    return out_p, out_j, out_x


def csr_outer_svec(A: DeviceCSR, vi: torch.Tensor, vx: torch.Tensor | None, length: int, v_dtype=None):
    """X %*% v for a device-resident one-column CSR X and a sparse vector, as the (p, i, x) tensors
    of a CSC with A.m rows and `length` columns: column vi[k] - 1 holds every non-empty row of X, ascending, times
    vx[k].  vi: sorted, unique 1-based int32 positions; vx: f64 values, int32 values (v_dtype MX_I32, the default, or
    MX_LGL; NA gives NA_real_), or None for an nsparseVector."""
    dev = A.indptr.device
    _one_column(A, "csr_outer_svec")
    vi, vx = _svec("csr_outer_svec", dev, vi, vx, (torch.float64, torch.int32))
    if v_dtype is None:
        v_dtype = _value_dtype(vx)
        if v_dtype == MX_LGL:           # an int32 vector is R integer unless the caller says logical
            v_dtype = _lib.MX_I32
    length, nv = int(length), int(vi.numel())
    if length < 0 or nv > length:
        raise ValueError("csr_outer_svec: more stored positions than the vector's length")
    ws = _workspace(dev, "mxd_csr_outer_svec_workspace_bytes", A.m, length)
    out_p = _int32(dev, length + 1)
    nonempty, k = _call("mxd_csr_outer_svec_count", A.m, A.nnz, _dp(A.indptr), _dp(A.values), _dp(vi), nv, length,
                        _dp(ws), _dp(out_p), cells=_COUNT * 2)
    out_i, out_x = _fill_pass(
        dev, k, (torch.int32, torch.float64),
        lambda oi, ox: _call("mxd_csr_outer_svec_fill", A.m, _dp(vi), nv, _dp(vx), v_dtype, length, nonempty, _dp(ws),
                             _dp(out_p), _dp(oi), _dp(ox)))
    return out_p, out_i, out_x


def rowvec_by_csc(v: torch.Tensor, A: DeviceCSR):
    """v %*% Y for a float32 row vector and a device-resident CSC Y held as DeviceCSR(p, i, x): A.m compressed columns
    over A.K rows, f64 values or None.  Returns float32[A.m]: per column the sum of x * v[i], each
    product in double, accumulated in float.  The row ids must lie below v.numel()."""
    dev = A.indptr.device
    if v.dtype != torch.float32 or v.dim() != 1 or v.device != dev or int(v.numel()) != A.K:
        raise ValueError(f"rowvec_by_csc: v must be a 1-d float32 tensor of Y's {A.K} rows on {dev}")
    if A.values is not None and A.values.dtype != torch.float64:
        raise ValueError("rowvec_by_csc: Y needs float64 values or none")
    out = torch.empty(A.m, dtype=torch.float32, device=dev)
    _call("mxd_rowvec_by_csc", A.m, A.nnz, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(v.contiguous()), _dp(out))
    return out


# ---- rbind / cbind: output sizes come from the operands' shapes, so nothing here waits for the device
_BIND_OUT = {_DGR: torch.float64, _LGR: torch.int32, _NGR: None}
_SVEC_KIND = {"d": _DSVEC, "i": _ISVEC, "l": _LSVEC, "n": _NSVEC}


def _matrix_kind(values) -> int:
    """dgR, lgR or ngR by the values tensor"""
    return {MX_F64: _DGR, MX_LGL: _LGR, MX_NONE: _NGR}[_value_dtype(values)]


def _vector_kind(vx, kind) -> int:
    """d / i / l / n sparseVector: `kind` when given, else by the values tensor (int32: logical)"""
    if kind is not None:
        return _SVEC_KIND[kind]
    return {MX_F64: _DSVEC, MX_LGL: _LSVEC, MX_NONE: _NSVEC}[_value_dtype(vx)]


def _bind_out_kind(kinds) -> int:
    """R/rbind.R:66-75: any numeric operand -> dgR, else any logical -> lgR, else ngR"""
    if any(k in (_DGR, _DSVEC, _ISVEC) for k in kinds):
        return _DGR
    return _LGR if any(k in (_LGR, _LSVEC) for k in kinds) else _NGR


def csr_rbind(items) -> DeviceCSR:
    """rbind of device-resident operands through mxd_csr_rbind_batch: two launches whatever len(items) is.  An item
    is a DeviceCSR (f64, int32 R-logical or no values) or a sparse vector (vi, vx, length) / (vi, vx, length, kind)
    with vi its int32 1-based indices, vx f64 / int32 / None and kind "d" / "i" / "l" / "n" (default by vx: int32 is
    logical).  The result has the value type R/rbind.R:66-75 gives and max-over-operands columns."""
    items = list(items)
    if not items:
        raise ValueError("csr_rbind: no operands")
    table = (_lib.RbindItem * len(items))()
    row = pos = ncol = 0
    kinds, dev = [], None
    for k, it in enumerate(items):
        if isinstance(it, DeviceCSR):
            kind, p, j, x, nr, nc = _matrix_kind(it.values), it.indptr, it.indices, it.values, it.m, it.K
        else:
            vi, vx, length = it[:3]
            kind, p, j, x, nr, nc = _vector_kind(vx, it[3] if len(it) > 3 else None), None, vi, vx, 1, int(length)
            if kind == _NSVEC:
                x = None
        _bind_indices(f"csr_rbind: operand {k}: indices must be contiguous int32, values as many as indices", j, x)
        dev = j.device if dev is None else dev
        n = int(j.numel())
        table[k] = _lib.RbindItem(kind, nr, None if p is None else p.data_ptr(), j.data_ptr(),
                                  None if x is None else x.data_ptr(), n, pos, row)
        kinds.append(kind)
        row, pos, ncol = row + nr, pos + n, max(ncol, nc)
    if row >= 2**31 - 1 or pos > 2**31 - 1:
        raise ValueError("csr_rbind: the result exceeds R's int32 index range")
    out_kind = _bind_out_kind(kinds)
    host = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)
    dtable = host.to(dev)
    out_p = _int32(dev, row + 1)
    out_j, out_x = _entries(dev, pos, torch.int32, _BIND_OUT[out_kind], floor=0)
    _call("mxd_csr_rbind_batch", _dp(dtable), len(items), out_kind, row, pos, _dp(out_p), _dp(out_j), _dp(out_x))
    return DeviceCSR(out_p, out_j, out_x, row, ncol, pos)


def csr_cbind(A: DeviceCSR, B: DeviceCSR) -> DeviceCSR:
    """cbind of two device-resident CSR operands of one value type (both f64, both int32 R-logical or both without
    values) through mxd_csr_cbind_shift: row r is A's row r, then B's with its columns moved up by A.K; the shorter
    operand contributes nothing past its end."""
    vd = _value_dtype(A.values)
    if _value_dtype(B.values) != vd:
        raise ValueError("csr_cbind: the operands must hold the same kind of values (convert one first)")
    if A.K + B.K > 2**31 - 1 or A.nnz + B.nnz > 2**31 - 1:
        raise ValueError("csr_cbind: the result exceeds R's int32 index range")
    dev = A.indptr.device
    m, nnz = max(A.m, B.m), A.nnz + B.nnz
    out_p = _int32(dev, m + 1)
    out_j, out_x = _entries(dev, nnz, torch.int32, _dtype(A.values), floor=0)
    _call("mxd_csr_cbind_shift", A.m, B.m, A.K, _dp(A.indptr), _dp(A.indices), _dp(A.values), _dp(B.indptr),
          _dp(B.indices), _dp(B.values), vd, nnz, _dp(out_p), _dp(out_j), _dp(out_x))
    return DeviceCSR(out_p, out_j, out_x, m, A.K + B.K, nnz)


def csr_cbind_svec(A: DeviceCSR, vi: torch.Tensor, vx: torch.Tensor | None, length: int, first: bool = False,
                   kind: str | None = None) -> DeviceCSR:
    """A with a sparse vector (vi: SORTED int32 1-based indices <= length, vx f64 / int32 / None, `kind` as in
    csr_rbind) as one more column, behind A's columns or (first=True) in front of them, through mxd_csr_cbind_svec.
    max(A.m, length) rows; the value type follows R/cbind.R:82-99."""
    _bind_indices("csr_cbind_svec: vi must be contiguous int32, vx as long as vi", vi, vx)
    xk, vk = _matrix_kind(A.values), _vector_kind(vx, kind)
    nv, length = int(vi.numel()), int(length)
    if nv > length or A.K + 1 > 2**31 - 1 or A.nnz + nv > 2**31 - 1:
        raise ValueError("csr_cbind_svec: more entries than cells, or a result beyond R's int32 index range")
    # R/cbind.R:82-99: pattern only from two patterns, logical when neither side is numeric
    out_kind = _NGR if (xk, vk) == (_NGR, _NSVEC) else _LGR if (xk in (_LGR, _NGR) and vk in (_LSVEC, _NSVEC)) else _DGR
    dev = A.indptr.device
    m, nnz = max(A.m, length), A.nnz + nv
    out_p = _int32(dev, m + 1)
    out_j, out_x = _entries(dev, nnz, torch.int32, _BIND_OUT[out_kind], floor=0)
    _call("mxd_csr_cbind_svec", A.m, A.K, _dp(A.indptr), _dp(A.indices), _dp(A.values), xk, _dp(vi),
          _dp(None if vk == _NSVEC else vx), vk, nv, length, int(bool(first)), out_kind, _dp(out_p), _dp(out_j),
          _dp(out_x))
    return DeviceCSR(out_p, out_j, out_x, m, A.K + 1, nnz)


# ---- reductions: one segmented reduction over entries, by rows or through the column order
REDUCE_OPS = {"sum": _lib.MX_RED_SUM, "abs_sum": _lib.MX_RED_ABS_SUM, "sq_sum": _lib.MX_RED_SQ_SUM,
              "abs_max": _lib.MX_RED_ABS_MAX}


def segment_reduce(values, op, segptr: torch.Tensor, nnz: int, perm=None, na_rm: bool = False, value_dtype=None):
    """out[s] = op over q in [segptr[s], segptr[s + 1]) of f(values[perm[q]]) through mxd_segment_reduce, as
    (float64 out, int32 skipped or None).  values: float64, int32 R logicals, or None (every entry is 1); op: a key of
    REDUCE_OPS; segptr: int32, nseg + 1 offsets.  No synchronisation."""
    if op not in REDUCE_OPS:
        raise ValueError(f"op must be one of {sorted(REDUCE_OPS)}, got {op!r}")
    dev = segptr.device
    nseg = int(segptr.numel()) - 1
    vd = _value_dtype(values) if value_dtype is None else value_dtype
    out, skipped = _entries(dev, nseg, torch.float64, torch.int32 if na_rm else None, floor=0)
    ws = _scratch(dev, 4 * _lib.load().mxd_compact_workspace_bytes(int(nnz)))
    _call("mxd_segment_reduce", REDUCE_OPS[op], _dp(values), vd, _dp(perm), int(nnz), _dp(segptr), nseg,
          int(bool(na_rm)), _dp(out), _dp(skipped), _dp(ws))
    return out, skipped


def row_reduce(A: DeviceCSR, op: str = "sum", na_rm: bool = False):
    """op over every row of a device-resident CSR (rowSums with "sum"): float64[A.m], or (result, skipped int32[A.m])
    with na_rm, which leaves NaN / NA entries out and counts them per row."""
    out, skipped = segment_reduce(A.values, op, A.indptr, A.nnz, None, na_rm)
    return (out, skipped) if na_rm else out


def col_reduce(A: DeviceCSR, op: str = "sum", na_rm: bool = False, order=None):
    """op over every column of a device-resident CSR (colSums with "sum"): float64[A.K], or (result, skipped) with
    na_rm.  order: the (perm, colptr) of DeviceCSR.column_order(), A's own (built once and cached) when None; pass the
    order of another DeviceCSR with the same indptr and indices (the values-only X * v shares them with X) and the
    sort is paid once per fit, not once per gradient."""
    perm, colptr = _order_of("col_reduce", A, order)
    out, skipped = segment_reduce(A.values, op, colptr, A.nnz, perm, na_rm)
    return (out, skipped) if na_rm else out


# ---- transposed products (include/mxgpu_tprod.h): X^T v fused on the tile scheme, X^T B through SpMM
def segment_dot(values, key: torch.Tensor, w: torch.Tensor, segptr: torch.Tensor, nnz: int, perm=None, out=None):
    """out[s] = sum over q in [segptr[s], segptr[s + 1]) of values[perm[q]] * w[key[q]] through mxd_segment_dot, float64.
    values: float64, or None (every entry is 1); key: int32[nnz] in segment order; w: float64.  Each product is rounded
    by itself and the sums are grouped as segment_reduce(..., "sum") groups them.  No synchronisation."""
    dev = segptr.device
    nseg = int(segptr.numel()) - 1
    if values is not None and values.dtype != torch.float64:
        raise ValueError(f"segment_dot: values must be float64 or None, got {values.dtype}")
    if w.dtype != torch.float64 or w.dim() != 1 or not w.is_contiguous() or w.device != dev:
        raise ValueError(f"segment_dot: w must be a contiguous 1-d float64 tensor on {dev}")
    if out is None:
        out, = _entries(dev, nseg, torch.float64, floor=0)
    elif tuple(out.shape) != (nseg,) or out.dtype != torch.float64 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"segment_dot: out must be a contiguous float64 tensor of {nseg} elements on {dev}")
    ws = _scratch(dev, 4 * _lib.load().mxd_compact_workspace_bytes(int(nnz)))
    _call("mxd_segment_dot", _dp(values), _value_dtype(values), _dp(perm), _dp(key), _dp(w), int(w.numel()), int(nnz),
          _dp(segptr), nseg, _dp(out), _dp(ws))
    return out


def spmv_t(A: DeviceCSR, v: torch.Tensor, out=None, order=None):
    """y = A^T @ v (crossprod(X, v)) for a float64 v of A.m elements: float64[A.K], through the column order (A's own
    cached one, or `order` as col_reduce takes it) and mxd_segment_dot.  Bit for bit the column sums of the written-out
    A * v[rows].  A's values are float64 or None (a pattern).  No synchronisation once the order is cached."""
    if v.dim() != 1 or int(v.numel()) != A.m:
        raise ValueError(f"spmv_t: v must have {A.m} elements, got {tuple(v.shape)}")
    perm, colptr = _order_of("spmv_t", A, order)
    rows = A.entry_rows(order)
    return segment_dot(A.values, rows, v, colptr, A.nnz, perm, out=out)


def spmm_t(A: DeviceCSR, B: torch.Tensor, out: torch.Tensor | None = None, colmajor: bool = False, order=None,
           **spmm_kwargs):
    """C = A^T @ B (crossprod(X, B)) with B (A.m x n) row-major: spmm(A.transposed(order), B, ...), the same kernels
    on the CSR of A^T, which costs one gather of the values once the order is cached."""
    return spmm(A.transposed(order), B, out=out, colmajor=colmajor, **spmm_kwargs)


# ---- sparse x sparse (include/mxgpu_spgemm.h): Gustavson by rows, count -> scan -> fill
def spgemm(A: DeviceCSR, B: DeviceCSR, uplo: str | None = None) -> DeviceCSR:
    """C = A @ B for two device-resident CSR operands through mxd_csr_spgemm_count / _fill: float64 values (int32 R
    logicals are read as 0 / 1 / NA_real_, a pattern as ones), rows sorted, nothing dropped.  A's rows may be unsorted
    and repeat a column; B's rows must not repeat one.  One host round trip (the entry count).  crossprod(X, Y) on
    resident operands is spgemm(X.transposed(), Y), which goes through X's cached column order.
    uplo "U" / "L": that triangle of the product alone, through mxd_csr_spgemm_tri_count / _fill (include/mxgpu_gram.h,
    DESIGN.md §4.24) with b_sorted = B.rows_sorted(); None makes exactly the calls above."""
    if A.K != B.m:
        raise ValueError(f"spgemm: A has {A.K} columns, B has {B.m} rows")
    dev = A.indptr.device
    # the mask's arguments stand behind the operands in both passes: none at all for the whole product
    tri, mask = ("_tri", (_uplo(uplo), int(B.rows_sorted()))) if uplo is not None else ("", ())
    ws = _workspace(dev, "mxd_csr_spgemm_workspace_bytes", A.m, B.K)
    out_p = _int32(dev, A.m + 1)
    _, k = _call(f"mxd_csr_spgemm{tri}_count", A.m, A.K, B.K, _dp(A.indptr), _dp(A.indices), A.nnz, _dp(B.indptr),
                 _dp(B.indices), B.nnz, *mask, _dp(out_p), _dp(ws), cells=_COUNT * 2)
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, torch.float64),
        lambda oj, ox: _call(f"mxd_csr_spgemm{tri}_fill", A.m, A.K, B.K, _dp(A.indptr), _dp(A.indices), _dp(A.values),
                             _value_dtype(A.values), _dp(B.indptr), _dp(B.indices), _dp(B.values),
                             _value_dtype(B.values), *mask, _dp(out_p), _dp(oj), _dp(ox), _dp(ws)))
    return DeviceCSR(out_p, out_j, out_x, A.m, B.K, k, _sorted=True)


def gram(A: DeviceCSR, trans: bool = True, uplo: str = "U", order=None) -> DeviceCSR:
    """The triangle `uplo` of the Gram product of a resident A: A^T A (A.K x A.K) with trans, A A^T (A.m x A.m) without,
    as a CSR that stores that triangle alone (what a dsRMatrix with this uplo holds).  It is spgemm(A.transposed(order),
    A, uplo) or spgemm(A, A.transposed(order), uplo): the transpose comes from the cached column order (or `order`, as
    col_reduce takes it), so a second call sorts nothing.  A must not repeat a cell inside a row."""
    At = A.transposed(order)
    return spgemm(At, A, uplo) if trans else spgemm(A, At, uplo)


def norm(A: DeviceCSR, type: str = "O") -> float:
    """norm(A, type) for type "O" (largest column sum of |x|), "I" (largest row sum), "F" (Frobenius) or "M" (largest
    |x|): the margin sums, then the same reduction over them as one "abs_max" segment.  Synchronises (a float)."""
    if type not in ("O", "I", "F", "M"):
        raise ValueError(f"norm: type must be one of 'O', 'I', 'F', 'M', got {type!r}")
    if A.m == 0 or A.K == 0 or A.nnz == 0:
        return 0.0
    dev = A.indptr.device

    def whole(values, op, n):
        segptr = torch.tensor([0, n], dtype=torch.int32, device=dev)
        return float(segment_reduce(values, op, segptr, n)[0].item())

    if type == "F":
        return float(np.sqrt(whole(A.values, "sq_sum", A.nnz)))
    if type == "M":
        return whole(A.values, "abs_max", A.nnz)
    sums = row_reduce(A, "abs_sum") if type == "I" else col_reduce(A, "abs_sum")
    return whole(sums, "abs_max", int(sums.numel()))


def diag(A: DeviceCSR):
    """diag(A) through mxd_csr_diag: the first stored (k, k) of every row k < min(A.m, A.K), 0 where there is none;
    float64 for numeric values, int32 R logicals for logical values (NA kept) and for a pattern (0 / 1)."""
    vd = _value_dtype(A.values)
    out, = _entries(A.indptr.device, min(A.m, A.K), torch.float64 if vd == MX_F64 else torch.int32, floor=0)
    _call("mxd_csr_diag", A.m, A.K, _dp(A.indptr), _dp(A.indices), _dp(A.values), vd, A.nnz, int(A.rows_sorted()),
          _dp(out))
    return out


# ---- symmetric / unit-triangular operands (include/mxgpu_sym.h) ----------------------------------
def _uplo(uplo: str) -> int:
    if uplo not in ("U", "L"):
        raise ValueError("uplo must be 'U' or 'L'")
    return _lib.MX_UPLO_UPPER if uplo == "U" else _lib.MX_UPLO_LOWER


def csr_triangle_check(A: DeviceCSR, uplo: str, strict: bool = False) -> int:
    """How many entries of the square A lie outside the triangle `uplo` (strict: or on the diagonal)."""
    ws = _scratch(A.indptr.device, 16)
    outside, = _call("mxd_csr_triangle_check", A.m, _dp(A.indptr), _dp(A.indices), A.nnz, _uplo(uplo),
                     int(bool(strict)), _dp(ws), cells=_COUNT)
    return outside


def csr_symmetric_count(A: DeviceCSR, uplo: str):
    """The count pass of the symmetric expansion: (out_indptr, workspace, nnz_out); the workspace holds the column
    order and the row ids that csr_symmetric_fill reads."""
    dev = A.indptr.device
    ws = _workspace(dev, "mxd_csr_sym_workspace_bytes", A.m, A.nnz)
    out_p = _int32(dev, A.m + 1)
    nnz_out, = _call("mxd_csr_symmetric_to_general_count", A.m, _dp(A.indptr), _dp(A.indices), A.nnz, _uplo(uplo),
                     _dp(out_p), _dp(ws), cells=_COUNT)
    return out_p, ws, nnz_out


def csr_symmetric_fill(A: DeviceCSR, uplo: str, out_p: torch.Tensor, ws: torch.Tensor, nnz_out: int,
                       out_j: torch.Tensor | None = None, out_x: torch.Tensor | None = None) -> DeviceCSR:
    """The fill pass: the general CSR, written into out_j / out_x when they are given."""
    dev = A.indptr.device
    if out_j is None:
        out_j, = _entries(dev, nnz_out, torch.int32)
    if out_x is None:
        out_x, = _entries(dev, nnz_out, _dtype(A.values))
    _call("mxd_csr_symmetric_to_general_fill", A.m, _dp(A.indptr), _dp(A.indices), _dp(A.values), _value_dtype(A.values),
          A.nnz, _uplo(uplo), _dp(out_p), nnz_out, _dp(out_j), _dp(out_x), _dp(ws))
    return DeviceCSR(out_p, out_j[:nnz_out], None if A.values is None else out_x[:nnz_out], A.m, A.K, nnz_out)


def csr_symmetric_to_general(A: DeviceCSR, uplo: str) -> DeviceCSR:
    """The general CSR of a symmetric A that stores the triangle `uplo`: count, scan, fill (mxgpu_sym.h)."""
    if A.m != A.K:
        raise ValueError("a symmetric matrix is square")
    out_p, ws, nnz_out = csr_symmetric_count(A, uplo)
    return csr_symmetric_fill(A, uplo, out_p, ws, nnz_out)


def csr_unit_triangular_to_general(A: DeviceCSR, uplo: str, out=None) -> DeviceCSR:
    """The general CSR of a strictly triangular A with an implied unit diagonal: one launch, no synchronisation.
    `out`: (indptr, indices, values) tensors to write into."""
    dev = A.indptr.device
    if A.m != A.K:
        raise ValueError("a triangular matrix is square")
    n_out = A.nnz + A.m
    if out is None:
        out = (_int32(dev, A.m + 1), *_entries(dev, n_out, torch.int32, _dtype(A.values)))
    out_p, out_j, out_x = out
    _call("mxd_csr_unit_triangular_to_general", A.m, _dp(A.indptr), _dp(A.indices), _dp(A.values),
          _value_dtype(A.values), A.nnz, _uplo(uplo), _dp(out_p), _dp(out_j), _dp(out_x))
    return DeviceCSR(out_p, out_j[:n_out], None if out_x is None else out_x[:n_out], A.m, A.K, n_out)


# ---- dense <-> compressed (include/mxgpu_dense.h) ---------------------------------------------------
def _colmajor_view(what: str, D: torch.Tensor):
    """(rows, cols, ld, transposed) under which the kernels read the 2-d tensor D as a column-major matrix without a
    copy: D itself when its rows are contiguous (stride (1, ld)), else its transpose when its columns are (a row-major
    D, stride (ld, 1)): the CSR arrays of a matrix are the CSC arrays of its transpose.  None when neither holds."""
    if D.dim() != 2:
        raise ValueError(f"{what}: the dense operand must be 2-d, got {D.dim()}-d")
    m, n = (int(s) for s in D.shape)
    for rows, cols, unit, ld, transposed in ((m, n, D.stride(0), D.stride(1), False),
                                             (n, m, D.stride(1), D.stride(0), True)):
        if (rows <= 1 or unit == 1) and (cols <= 1 or ld >= max(rows, 1)):
            return rows, cols, (int(ld) if cols > 1 else max(rows, 1)), transposed
    return None


def dense_to_csr(D: torch.Tensor, by_col: bool = False, out_kind: int = MX_F64, logical: bool = False,
                 col_splits: int = 0) -> DeviceCSR:
    """The CSR arrays (by_col: the CSC arrays, as the DeviceCSR of D^T) of a dense m x n tensor through
    mxd_dense_to_csr_count / _fill: the cells that are not zero, NaN and NA kept, -0.0 dropped, rows sorted.  D is
    float64, float32, int32 (R integers, or R logicals with `logical`) or bool, column- or row-major with any leading
    dimension (read in place); anything else is copied once.  out_kind: MX_F64 (values as f64, NA -> NA_real_), MX_LGL
    (int32 R logicals, NaN -> NA) or MX_NONE (a pattern)."""
    if out_kind not in (MX_F64, MX_LGL, MX_NONE):
        raise ValueError("dense_to_csr: out_kind must be MX_F64, MX_LGL or MX_NONE")
    if D.dim() != 2:
        raise ValueError(f"dense_to_csr: the dense operand must be 2-d, got {D.dim()}-d")
    m, n = (int(s) for s in D.shape)
    X, kind = _dense_kind("dense_to_csr", D, logical)
    view = _colmajor_view("dense_to_csr", X)
    if view is None:
        X = X.t().contiguous().t()
        view = _colmajor_view("dense_to_csr", X)
    rows, cols, ld, transposed = view
    col = int(bool(by_col) != transposed)
    dev = X.device
    nseg, nother = (n, m) if by_col else (m, n)
    ws = _workspace(dev, "mxd_dense_to_csr_workspace_bytes", rows, cols, col, int(col_splits))
    out_p = _int32(dev, nseg + 1)
    k, = _call("mxd_dense_to_csr_count", rows, cols, _dp(X), ld, kind, col, int(col_splits), _dp(out_p), _dp(ws),
               cells=_COUNT)
    vdt = {MX_F64: torch.float64, MX_LGL: torch.int32, MX_NONE: None}[out_kind]
    out_j, out_x = _fill_pass(
        dev, k, (torch.int32, vdt),
        lambda oj, ox: _call("mxd_dense_to_csr_fill", rows, cols, _dp(X), ld, kind, col, int(col_splits), _dp(out_p),
                             _dp(ws), _dp(oj), _dp(ox), out_kind))
    return DeviceCSR(out_p, out_j, out_x, nseg, nother, k, _sorted=True)


def csr_to_dense(A: DeviceCSR, by_col: bool = False, out: torch.Tensor | None = None, logical: bool = False,
                 flag: torch.Tensor | None = None, col_splits: int = 0) -> torch.Tensor:
    """A as a dense tensor through mxd_csr_to_dense: A.m x A.K for CSR arrays, A.K x A.m with by_col (A then holds the
    CSC arrays: A.m columns, indices below A.K).  float64 (NA -> NA_real_, a pattern entry -> 1.0), or int32 R logicals
    with `logical`.  `out`: a tensor of that shape and dtype, column- or row-major with any leading dimension, of which
    only the cells of the matrix are written; by default a new column-major one.  Every row of A must be strictly
    ascending and in range: the kernel sets the int32 device cell `flag` otherwise.  With a caller's `flag` (zeroed by
    the caller) nothing is read back and the call does not synchronise; without one the flag is read and a flagged
    operand raises ValueError."""
    vd = _value_dtype(A.values)
    dt = torch.int32 if logical else torch.float64
    dev = A.indptr.device
    shape = (A.K, A.m) if by_col else (A.m, A.K)
    if out is None:
        out = torch.empty(shape[::-1], dtype=dt, device=dev).t()
    elif tuple(out.shape) != shape or out.dtype != dt or out.device != dev:
        raise ValueError(f"csr_to_dense: out must be a {shape} {dt} tensor on {dev}, got {tuple(out.shape)} {out.dtype} "
                         f"on {out.device}")
    view = _colmajor_view("csr_to_dense", out)
    if view is None:
        raise ValueError(f"csr_to_dense: out must have contiguous rows or contiguous columns, got strides {out.stride()}")
    _, _, ld, transposed = view
    own = flag is None
    if own:
        flag = _int32(dev, 1).zero_()
    _call("mxd_csr_to_dense", A.m, A.K, _dp(A.indptr), _dp(A.indices), _dp(A.values), vd, int(bool(by_col) != transposed),
          int(col_splits), _dp(out), ld, MX_LGL if logical else MX_F64, _dp(flag))
    if own and int(flag.item()):
        raise ValueError("csr_to_dense: the indices of a row are not strictly ascending or not in range")
    return out
