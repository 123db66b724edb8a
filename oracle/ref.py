"""ctypes front end of the reference's own compiled C++ (oracle/_ref/libmxref.so, `make -C oracle ref`).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tests/golden/make_reference_golden.py, never by matrixextra_amd/.

Every R-callable entry point of the reference's matmul / operators / slice / slice_coo / misc / cbind / rbind files
is reachable as an attribute of this module under its own name and argument order, which are also those of
oracle/oracle.py and matrixextra_amd/exports.py, so a test can swap `O` for `Ref`.  Arguments are cast by the
signature that the driver reports: int32 for integer and logical vectors, float64 for numeric ones, Fortran order
for matrices; a float32 array stands for the `float32@Data` integer bits and float32 comes back.  Results are what
the R side receives: numpy arrays, a dict for a list, str, bool / int / float.

Aliasing is kept: arguments that are one numpy buffer reach the reference as one R vector, a result vector that IS
an argument vector comes back as that argument object, and vectors that a function changes in place are copied back
into writable int32 / float64 arguments.

Known hazard: `gemm_csr_drm_as_dcm` allocates `ldc` scratch entries and uses `ldb` of them (matmul.cpp:176,179),
a heap overflow when n > m.  tcrossprod_csr_dense_* (the column-major CSR x dense exports) therefore refuse a dense
operand with more rows than the sparse one here; compare those shapes through the oracle only.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_ref", "libmxref.so")
_FLAGS = os.path.join(_HERE, "_ref", "flags.txt")
REFERENCE = os.environ.get("MX_REFERENCE", "/root/reference")

LGLSXP, INTSXP, REALSXP, STRSXP, VECSXP, S4SXP = 10, 13, 14, 16, 19, 25


class RefError(RuntimeError):
    """An Rcpp::stop() (or any C++ exception) inside the reference."""


def sources_present() -> bool:
    return os.path.exists(os.path.join(REFERENCE, "src", "operators.cpp"))


def available() -> bool:
    return os.path.exists(_SO)


def build() -> str:
    """Runs the `ref` target when the reference's sources are there; otherwise leaves what exists alone."""
    if sources_present():
        subprocess.check_call(["make", "-C", _HERE, "-j", str(min(16, os.cpu_count() or 1)), "ref",
                               f"REFERENCE={REFERENCE}"], stdout=subprocess.DEVNULL)
    return _SO


def compile_flags() -> str:
    with open(_FLAGS) as f:
        return f.read().strip()


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_SO)
        for name in ("mxref_vector", "mxref_matrix", "mxref_string", "mxref_container", "mxref_data", "mxref_item"):
            getattr(L, name).restype = C.c_void_p
        for name in ("mxref_chars", "mxref_item_name", "mxref_signature", "mxref_function_name"):
            getattr(L, name).restype = C.c_char_p
        for name in ("mxref_length", "mxref_live_objects", "mxref_function_count"):
            getattr(L, name).restype = C.c_long
        L.mxref_vector.argtypes = [C.c_int, C.c_void_p, C.c_long]
        L.mxref_matrix.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.mxref_container.argtypes = [C.c_int, C.c_char_p]
        L.mxref_container_add.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        for name in ("mxref_type", "mxref_length", "mxref_data", "mxref_nrow", "mxref_ncol", "mxref_chars",
                     "mxref_free"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.mxref_item_name.argtypes = [C.c_void_p, C.c_long]
        L.mxref_item.argtypes = [C.c_void_p, C.c_long]
        L.mxref_call.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
        _lib = L
    return _lib


def functions():
    L = lib()
    return sorted(L.mxref_function_name(i).decode() for i in range(L.mxref_function_count()))


def signature(name: str):
    s = lib().mxref_signature(name.encode())
    return None if s is None else s.decode()


def live_objects() -> int:
    return int(lib().mxref_live_objects())


_VEC = {"I": (INTSXP, np.int32), "L": (LGLSXP, np.int32), "N": (REALSXP, np.float64)}
_MAT = {"J": (INTSXP, np.int32), "K": (LGLSXP, np.int32), "M": (REALSXP, np.float64)}


def _cast(a, dt):
    a = np.asarray(a)
    if a.dtype == np.float32 and dt == np.int32:
        return np.ascontiguousarray(a).view(np.int32)          # float32@Data: the bits, as R's `float` package
    if a.dtype == np.bool_ and dt == np.int32:
        return a.astype(np.int32)
    return a.astype(dt, copy=False)


class _Call:
    """The handles of one call: made once per distinct numpy buffer, freed together."""

    def __init__(self):
        self.handles = []
        self.by_buffer = {}      # (address, size, R type) -> (handle, argument object)
        self.vectors = []        # (handle, argument object, R type)
        self.alive = []          # the cast arrays, so that no address is reused while by_buffer is in use

    def keep(self, h):
        if not h:
            raise MemoryError("the reference stand-in could not allocate")
        self.handles.append(h)
        return h

    def vector(self, obj, kind):
        L = lib()
        if kind in _VEC:
            rt, dt = _VEC[kind]
            a = _cast(obj, dt)
            a = np.ascontiguousarray(a.reshape(-1, order="F") if a.ndim == 2 else a).reshape(-1)   # a matrix is its columns
            self.alive.append(a)
            key = (a.__array_interface__["data"][0], a.size, rt) if a.size else None
            if key is not None and key in self.by_buffer:
                return self.by_buffer[key][0]
            h = self.keep(L.mxref_vector(rt, a.ctypes.data, a.size))
        else:
            rt, dt = _MAT[kind]
            a = _cast(obj, dt)
            if a.ndim != 2:
                raise ValueError("a matrix argument must be two-dimensional")
            a = np.asfortranarray(a)
            key = None
            h = self.keep(L.mxref_matrix(rt, a.ctypes.data, a.shape[0], a.shape[1]))
        if key is not None:
            self.by_buffer[key] = (h, obj)
        self.vectors.append((h, obj, rt))
        return h

    def scalar(self, v, kind):
        L = lib()
        if kind == "d":
            a = np.array([v], dtype=np.float64)
            return self.keep(L.mxref_vector(REALSXP, a.ctypes.data, 1))
        a = np.array([int(v)], dtype=np.int32)
        return self.keep(L.mxref_vector(LGLSXP if kind == "b" else INTSXP, a.ctypes.data, 1))

    def s4(self, classes, slots):
        L = lib()
        h = self.keep(L.mxref_container(S4SXP, " ".join(classes).encode()))
        for name, (kind, value) in slots.items():
            L.mxref_container_add(h, name.encode(), self.vector(value, kind))
        return h

    def free(self):
        L = lib()
        for h in self.handles:
            L.mxref_free(h)
        self.handles = []


def _array(h, as_float32):
    L = lib()
    t, n = L.mxref_type(h), L.mxref_length(h)
    dt = np.float64 if t == REALSXP else np.int32
    out = np.empty(n, dtype=dt)
    if n:
        C.memmove(out.ctypes.data, L.mxref_data(h), out.nbytes)
    if as_float32 and t == INTSXP:
        out = out.view(np.float32)
    nr, nc = L.mxref_nrow(h), L.mxref_ncol(h)
    if nr >= 0:
        out = out.reshape((nr, nc), order="F")
    return out


def _value(h, call, kind, as_float32):
    L = lib()
    t = L.mxref_type(h)
    if t == STRSXP:
        return L.mxref_chars(h).decode()
    if t == VECSXP:
        out = {}
        for i in range(L.mxref_length(h)):
            item = L.mxref_item(h, i)
            try:
                out[L.mxref_item_name(h, i).decode()] = _value(item, call, "", False)
            finally:
                L.mxref_free(item)
        return out
    if kind in ("b", "i", "d"):
        v = _array(h, False)[0]
        return bool(v) if kind == "b" else (int(v) if kind == "i" else float(v))
    for hh, obj, _rt in call.vectors:      # the reference returned one of its arguments
        if hh == h:
            return obj
    return _array(h, as_float32)


def call(name: str, *args):
    """Calls the reference's `name`.  Raises RefError with the message of an Rcpp::stop()."""
    L = lib()
    sig = signature(name)
    if sig is None:
        raise AttributeError(f"the reference has no entry point {name!r}")
    rkind, akinds = sig[0], sig[1:]
    if len(args) != len(akinds):
        raise TypeError(f"{name} takes {len(akinds)} arguments, {len(args)} given")
    as_float32 = any(isinstance(a, np.ndarray) and a.dtype == np.float32 for a in args)
    c = _Call()
    result = C.c_void_p()
    try:
        hs = []
        for a, k in zip(args, akinds):
            if k in _VEC or k in _MAT:
                hs.append(c.vector(a, k))
            elif k in "ibd":
                hs.append(c.scalar(a, k))
            elif k == "S":
                hs.append(c.keep(L.mxref_string(str(a).encode())))
            else:
                raise TypeError(f"{name}: argument kind {k!r} needs a wrapper of its own")
        arr = (C.c_void_p * max(len(hs), 1))(*hs)
        err = C.create_string_buffer(512)
        status = L.mxref_call(name.encode(), arr, len(hs), C.byref(result), err, len(err))
        if status != 0:
            raise RefError(err.value.decode())
        for h, obj, rt in c.vectors:       # in-place functions: hand the changed vectors back
            want = np.float64 if rt == REALSXP else np.int32
            if isinstance(obj, np.ndarray) and obj.dtype == want and obj.flags.writeable and obj.size:
                new = _array(h, False).reshape(obj.shape, order="F")
                if new.tobytes("F") != obj.tobytes("F"):
                    obj[...] = new
        if not result:
            return None
        return _value(result.value, c, rkind, as_float32)
    finally:
        if result:
            L.mxref_free(result)
        c.free()


# ----------------------------------------------------------------------------- wrappers whose Python shape is not the
#                                                                               plain export (as in oracle.py)
def _guard_n_le_m(X_indptr, Y):
    if np.asarray(Y).shape[0] > np.asarray(X_indptr).size - 1:
        raise ValueError("tcrossprod_csr_dense through the reference needs n <= m (scratch overflow, matmul.cpp:176)")


def tcrossprod_csr_dense_numeric(X_indptr, X_indices, X_values, Y_colmajor, nthreads=1):
    _guard_n_le_m(X_indptr, Y_colmajor)
    return call("tcrossprod_csr_dense_numeric", X_indptr, X_indices, X_values, Y_colmajor, nthreads)


def tcrossprod_csr_dense_float32(X_indptr, X_indices, X_values, Y_colmajor, nthreads=1):
    _guard_n_le_m(X_indptr, Y_colmajor)
    return call("tcrossprod_csr_dense_float32", X_indptr, X_indices, X_values,
                np.asarray(Y_colmajor, dtype=np.float32), nthreads)


def matmul_dense_csc_numeric(X, p, i, x, nthreads=1):
    return call("matmul_dense_csc_numeric", X, p, i, x, nthreads)


def matmul_dense_csc_float32(X, p, i, x, nthreads=1):
    return call("matmul_dense_csc_float32", np.asarray(X, dtype=np.float32), p, i, x, nthreads)


def tcrossprod_dense_csr_numeric(X, p, j, x, nthreads=1, ncols_Y=0):
    return call("tcrossprod_dense_csr_numeric", X, p, j, x, nthreads, ncols_Y)


def tcrossprod_dense_csr_float32(X, p, j, x, nthreads=1, ncols_Y=0):
    return call("tcrossprod_dense_csr_float32", np.asarray(X, dtype=np.float32), p, j, x, nthreads, ncols_Y)


def _with_threads(name, float32_arg=None):
    def f(*args, nthreads=1):
        args = list(args)
        if float32_arg is not None:
            args[float32_arg] = np.asarray(args[float32_arg], dtype=np.float32)
        if len(args) == len(signature(name)) - 1:
            return call(name, *args)
        return call(name, *args, nthreads)
    f.__name__ = name
    return f


for _n in ("numeric", "integer", "logical"):
    globals()[f"matmul_csr_dvec_{_n}"] = _with_threads(f"matmul_csr_dvec_{_n}")
    globals()[f"matmul_csr_svec_{_n}"] = _with_threads(f"matmul_csr_svec_{_n}")
matmul_csr_dvec_float32 = _with_threads("matmul_csr_dvec_float32", 3)
matmul_csr_svec_float32 = _with_threads("matmul_csr_svec_float32", 4)
matmul_csr_svec_binary = _with_threads("matmul_csr_svec_binary")


def sort_sparse_indices(indptr, indices, values=None):
    """As oracle.sort_sparse_indices: sorted COPIES (sort_sparse_indices_{numeric,logical,binary}, misc.cpp)."""
    j = np.array(indices, dtype=np.int32, copy=True)
    if values is None:
        call("sort_sparse_indices_binary", indptr, j)
        return j, None
    v = np.array(values, copy=True)
    if v.dtype == np.float64:
        call("sort_sparse_indices_numeric", indptr, j, v)
    else:
        v = v.astype(np.int32)
        call("sort_sparse_indices_logical", indptr, j, v)
    return j, v


def check_indices_are_sorted(indptr, indices) -> bool:
    """The per-row check_is_sorted of misc.cpp:118-128, through the export that takes one vector."""
    p, j = np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32)
    return all(call("check_is_sorted", j[p[r]:p[r + 1]].copy()) for r in range(p.size - 1))


def reverse_columns_inplace(indptr, indices, values, ncol):
    """As oracle.reverse_columns_inplace: changes `indices` / `values` in place."""
    if values is None:
        call("reverse_columns_inplace_binary", indptr, indices, np.zeros(0), ncol)
    elif values.dtype == np.float64:
        call("reverse_columns_inplace_numeric", indptr, indices, values, ncol)
    else:
        call("reverse_columns_inplace_logical", indptr, indices, values, ncol)


def reverse_columns_inplace_binary(indptr, indices, ncol):
    call("reverse_columns_inplace_binary", indptr, indices, np.zeros(0), ncol)


_MATRIX_CLASS = {0: ("dgRMatrix", "N"), 1: ("lgRMatrix", "L"), 2: ("ngRMatrix", None)}
_VECTOR_CLASS = {3: ("dsparseVector", "N"), 4: ("isparseVector", "I"), 5: ("lsparseVector", "L"),
                 6: ("nsparseVector", None)}


def concat_csr_batch(objects, out_kind):
    """As oracle.concat_csr_batch: objects = [(in_kind, indptr|None, indices, values|None, nrows)], kinds 0 dgR,
    1 lgR, 2 ngR, 3..6 d/i/l/n sparseVector with 1-based indices.  Builds the S4 objects the reference reads."""
    L = lib()
    c = _Call()
    try:
        lst = c.keep(L.mxref_container(VECSXP, None))
        for kind, p, j, x, nr in objects:
            if kind <= 2:
                cls, vk = _MATRIX_CLASS[kind]
                slots = {"p": ("I", p), "j": ("I", j), "Dim": ("I", np.array([nr, 0], dtype=np.int32))}
            else:
                cls, vk = _VECTOR_CLASS[kind]
                slots = {"i": ("I", j)}
            if vk is not None:
                slots["x"] = (vk, x)
            L.mxref_container_add(lst, b"", c.s4([cls], {k: (kk, np.array(v, copy=True)) for k, (kk, v) in slots.items()}))
        nrows = sum(o[4] if o[0] <= 2 else 1 for o in objects)
        nnz = sum(np.asarray(o[2]).size for o in objects)
        cls, vk = _MATRIX_CLASS[out_kind]
        indptr, indices = np.zeros(nrows + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
        values = None if vk is None else np.zeros(nnz, dtype=np.float64 if vk == "N" else np.int32)
        slots = {"p": ("I", indptr), "j": ("I", indices)}
        if vk is not None:
            slots["x"] = (vk, values)
        out = c.s4([cls], slots)
        arr = (C.c_void_p * 2)(lst, out)
        result, err = C.c_void_p(), C.create_string_buffer(512)
        status = L.mxref_call(b"concat_csr_batch", arr, 2, C.byref(result), err, len(err))
        if result:
            L.mxref_free(result)
        if status != 0:
            raise RefError(err.value.decode())
        got = {}
        for h, obj, _rt in c.vectors:
            for key, target in (("indptr", indptr), ("indices", indices), ("values", values)):
                if obj is target:
                    got[key] = _array(h, False)
        got.setdefault("values", None)
        return got
    finally:
        c.free()


def __getattr__(name):
    if name.startswith("_") or not available() or signature(name) is None:
        raise AttributeError(name)

    def f(*args):
        return call(name, *args)
    f.__name__ = name
    return f


if __name__ == "__main__":
    build()
    print(f"{_SO}: {len(functions())} entry points, flags: {compile_flags()}", file=sys.stderr)
