"""ctypes binding of libmxgpu.so — the only way Python reaches the HIP kernels.

There is no fallback: if the shared library is missing or fails to load, or a
call reports an error, an exception is raised.  `torch` is imported first when
it is installed so that the library binds to the same HIP runtime instance
(same `libamdhip64.so.7` SONAME) as torch's allocator and RCCL — device
pointers of torch tensors can then be handed to the mxd_* entry points.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmxgpu.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu.h")
REDUCE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu_reduce.h")
SYM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu_sym.h")
TPROD_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu_tprod.h")
SPGEMM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu_spgemm.h")
GRAM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu_gram.h")
DENSE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mxgpu_dense.h")


class MxError(RuntimeError):
    """An mx_* / mxd_* call returned non-zero (the .Call shim would Rf_error here)."""


# ---- include/mxgpu.h is the one declaration of the ABI: signatures, constants and structs are read from it ----------
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}
_INT = r"-?(?:0x[0-9a-fA-F]+|\d+)"


class Header(NamedTuple):
    functions: dict     # name -> (restype, (argtypes...)) as ctypes types
    constants: dict     # enumerators and integer #defines, by their C names
    structs: dict       # typedef struct {...} name; -> ctypes.Structure class


def _ctype(spelling: str, where: str, returned: bool = False):
    """The ctypes type of one C type.  Every pointer is a c_void_p, which takes None, an address, a c_void_p, a ctypes
    array and byref(...) alike; only a returned `const char *` is a c_char_p."""
    t = re.sub(r"\s*\*\s*", "*", " ".join(spelling.split()))
    if returned and t == "const char*":
        return C.c_char_p
    if not returned and t.endswith("*"):
        return C.c_void_p
    if t not in _SCALARS:
        raise MxError(f"include/mxgpu.h: {where}: no ctypes mapping for type '{t}'")
    return _SCALARS[t]


def _struct(name: str, body: str):
    fields = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        first, *rest = (d.strip() for d in member.split(","))
        base, first = re.match(r"(.*?)(\**\s*\w+)$", first).groups()  # "const void *x" -> "const void ", "*x"
        for d in (first, *rest):                                        # "int lo, hi, reversed" declares three
            field = d.lstrip("* ")
            fields.append((field, _ctype(base + "*" * d.count("*"), f"{name}.{field}")))
    return type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"{name} (include/mxgpu.h)."})


def parse_header(text: str) -> Header:
    """Everything the binding needs from the text of mxgpu.h.  Strict: a type outside the map, an enumerator without
    a value, or an mx_* / mxd_* name followed by `(` that is not a plain prototype, raises MxError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    defines = re.findall(rf"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+({_INT})[ \t]*$", text, flags=re.M)
    constants = {name: int(value, 0) for name, value in defines}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for body, name in re.findall(r"typedef\s+enum\s*\{([^}]*)\}\s*(\w+)\s*;", text):
        for item in filter(None, (e.strip() for e in body.split(","))):
            m = re.fullmatch(rf"(\w+)\s*=\s*({_INT})", item)
            if m is None:
                raise MxError(f"include/mxgpu.h: enum {name}: '{item}' carries no explicit integer value")
            constants[m.group(1)] = int(m.group(2), 0)
    structs = {name: _struct(name, body)
               for body, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;", text)}
    functions = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s*]*?)\b(mxd?_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        named = (re.fullmatch(r"(.*[\s*])\w+", p) for p in params)          # "const void *B" -> "const void *"
        argtypes = tuple(_ctype(m.group(1) if m else p, f"{name}(), parameter {k + 1}")
                         for k, (p, m) in enumerate(zip(params, named)))
        functions[name] = (_ctype(ret, f"{name}(), return type", returned=True), argtypes)
    stray = sorted(set(re.findall(r"\b(mxd?_\w+)\s*\(", text)) - set(functions))
    if stray:
        raise MxError(f"include/mxgpu.h: not a prototype the binding can read: {stray}")
    return Header(functions, constants, structs)


def _read_header(path: str = HEADER_PATH) -> Header:
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise MxError(f"{path} not readable ({e}): the ctypes signatures, constants and structs of "
                      "libmxgpu.so are bound from it") from e


HEADER = _read_header()
globals().update(HEADER.constants)        # MX_F64 ... MX_NONE, MX_OP_*, MX_KEEP_*, MX_ALIAS_ALL, MXGPU_ABI_VERSION, ...
# the reduction family has a header and a table of its own (include/mxgpu_reduce.h), bound on the same library;
# HEADER and declared_symbols() stay what include/mxgpu.h declares
REDUCE_HEADER = _read_header(REDUCE_HEADER_PATH)
globals().update(REDUCE_HEADER.constants)  # MX_RED_SUM, MX_RED_ABS_SUM, MX_RED_SQ_SUM, MX_RED_ABS_MAX
# so has the structured-matrix family (include/mxgpu_sym.h): symmetric / unit-triangular expansion, triangle check
SYM_HEADER = _read_header(SYM_HEADER_PATH)
globals().update(SYM_HEADER.constants)     # MX_UPLO_UPPER, MX_UPLO_LOWER
# and the transposed products (include/mxgpu_tprod.h): the segmented dot, the transpose by a column order, X^T v, X^T B
TPROD_HEADER = _read_header(TPROD_HEADER_PATH)
# and the sparse x sparse product (include/mxgpu_spgemm.h): limits, count and fill at device level, one export
SPGEMM_HEADER = _read_header(SPGEMM_HEADER_PATH)
# and its one-triangle form with the Gram products on it (include/mxgpu_gram.h): count and fill behind a mask, one export
GRAM_HEADER = _read_header(GRAM_HEADER_PATH)
# and the dense <-> compressed conversions (include/mxgpu_dense.h): count, fill and the scatter at device level, two exports
DENSE_HEADER = _read_header(DENSE_HEADER_PATH)
# mx_dvec_op, by R's operator
MX_DV_OPS = {"*": HEADER.constants["MX_DV_MULTIPLY"], "^": HEADER.constants["MX_DV_POWERTO"],
             "/": HEADER.constants["MX_DV_DIVIDE"], "%%": HEADER.constants["MX_DV_DIVREST"],
             "%/%": HEADER.constants["MX_DV_INTDIV"]}
ResultInfo = HEADER.structs["mx_result_info"]
CooAxis = HEADER.structs["mx_coo_axis"]
RbindInput = HEADER.structs["mx_rbind_input"]
RbindItem = HEADER.structs["mx_rbind_item"]

_lib = None


def declared_symbols() -> list[str]:
    """Every function name include/mxgpu.h declares (used by the export test)."""
    return sorted(HEADER.functions)


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MxError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C matrixextra_amd/csrc`. There is no CPU fallback.")
    try:  # share torch's HIP runtime when torch is present (see module docstring)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the plain C-ABI
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for header, path in ((HEADER, "include/mxgpu.h"), (REDUCE_HEADER, "include/mxgpu_reduce.h"),
                         (SYM_HEADER, "include/mxgpu_sym.h"), (TPROD_HEADER, "include/mxgpu_tprod.h"),
                         (SPGEMM_HEADER, "include/mxgpu_spgemm.h"), (GRAM_HEADER, "include/mxgpu_gram.h"),
                         (DENSE_HEADER, "include/mxgpu_dense.h")):
        missing = [name for name in header.functions if not hasattr(lib, name)]
        if missing:
            raise MxError(f"libmxgpu.so lacks symbols declared in {path}: {missing}")
        for name, (restype, argtypes) in header.functions.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    if lib.mx_abi_version() != HEADER.constants["MXGPU_ABI_VERSION"]:
        raise MxError("libmxgpu.so ABI version mismatch")
    _lib = lib
    return lib


def last_row_launch() -> tuple[str, int]:
    """(label, lanes per row) of the last row-group kernel this thread launched (mxd_last_row_launch)."""
    what, G = C.c_char_p(), C.c_int(0)
    check(load().mxd_last_row_launch(C.byref(what), C.byref(G)))
    return (what.value or b"").decode(), G.value


def check(rc: int) -> None:
    if rc != 0:
        raise MxError(load().mx_last_error().decode("utf-8", "replace"))


def ptr(a):
    """void* of a numpy array (None -> NULL)."""
    return None if a is None else C.c_void_p(a.ctypes.data)


def device_count() -> int:
    n = C.c_int(0)
    check(load().mx_device_count(C.byref(n)))
    return n.value


def device_name() -> str:
    buf = C.create_string_buffer(256)
    check(load().mx_device_name(buf, 256))
    return buf.value.decode()
