"""Replays one recorded call of the export-level C-ABI (mx_*) through ctypes.  Shared by the makers of
tests/golden/export_host_behaviour.json and tests/golden/export_result_shapes.json and by the tests that hold a build
to those records, so that the record and the replay cannot drift apart.

A call is [function name, [argument, ...]].  An argument is
    an int                      a scalar
    None                        a null pointer
    ["i32" | "u32" | "u64", [...]]   an input array; float32 / float64 travel as their u32 / u64 bit patterns
    ["out", n_bytes]            an output buffer, pre-filled with SENTINEL so that "untouched" and "zeroed" differ
    ["same", k]                 the very pointer of argument k (the pointer-identity paths)
    ["rbind", [[kind, indptr, indices, values, nrows, nnz], ...]]   an mx_rbind_input array (members as above)
    "res" | "info"              the mx_result ** / mx_result_info * of a *_begin export
The outcome is {"status", "error" (non-zero status only), "outs" (hex of every output buffer)} and, for a *_begin
call that succeeded, "info" (the five mx_result_info fields) and "indptr" / "indices" / "values", what
mx_result_finish wrote into sentinel-filled vectors of the reported lengths, as int32 / uint32 / uint64 bit patterns."""
import ctypes as C

import numpy as np

from matrixextra_amd import _lib

SENTINEL = 0xA5
_DTYPES = {"i32": np.int32, "u32": np.uint32, "u64": np.uint64}
INFO_FIELDS = ("indptr_len", "nnz", "values_len", "values_dtype", "alias_structure")


def _array(spec, keep):
    if spec is None:
        return None
    a = np.array(spec[1], dtype=_DTYPES[spec[0]])
    keep.append(a)
    return C.c_void_p(a.ctypes.data)


def run_call(fn_name, args):
    lib = _lib.load()
    keep, outs, passed = [], [], []
    res, info = C.c_void_p(), _lib.ResultInfo()
    begun = False
    for a in args:
        if a is None or isinstance(a, int):
            passed.append(a)
        elif a == "res":
            passed.append(C.byref(res))
            begun = True
        elif a == "info":
            passed.append(C.byref(info))
        elif a[0] == "out":
            buf = np.full(a[1], SENTINEL, dtype=np.uint8)
            outs.append(buf)
            passed.append(C.c_void_p(buf.ctypes.data))
        elif a[0] == "same":
            passed.append(passed[a[1]])
        elif a[0] == "rbind":
            objs = (_lib.RbindInput * max(len(a[1]), 1))()
            for o, (kind, indptr, indices, values, nrows, nnz) in zip(objs, a[1]):
                o.kind, o.nrows, o.nnz = kind, nrows, nnz
                o.indptr, o.indices, o.values = _array(indptr, keep), _array(indices, keep), _array(values, keep)
            keep.append(objs)
            passed.append(C.cast(objs, C.c_void_p))
        else:
            passed.append(_array(a, keep))
    status = getattr(lib, fn_name)(*passed)
    got = {"status": status, "outs": [o.tobytes().hex() for o in outs]}
    if status < 0 or (status != 0 and fn_name != "mx_dense_by_svec_route"):    # the route's 1..3 are answers
        got["error"] = lib.mx_last_error().decode()
    elif begun:
        got["info"] = [int(getattr(info, f)) for f in INFO_FIELDS]
        wide = info.values_dtype == _lib.MX_F64
        indptr = np.full(info.indptr_len, SENTINEL, dtype=np.uint8).repeat(4).view(np.int32)
        indices = np.full(info.nnz, SENTINEL, dtype=np.uint8).repeat(4).view(np.int32)
        values = np.full(info.values_len, SENTINEL, dtype=np.uint8).repeat(8 if wide else 4).view(
            np.uint64 if wide else np.uint32)
        got["finish"] = lib.mx_result_finish(res, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(values))
        got["indptr"], got["indices"], got["values"] = indptr.tolist(), indices.tolist(), values.tolist()
    return got
