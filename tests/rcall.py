"""The .Call shim (matrixextra_amd/csrc/r_shim.cpp) as a Python module under the reference's function names.

tests/_build/libmxgpu_rshim.so is the shim compiled against the stand-in for R's C API (tests/rstub) and linked to
libmxgpu.so; libmxgpu_rshim_fake.so is the same shim over a generated fake of the C-ABI.  `rcall.<routine>(*args)`
(module level: the real library) and `rcall.load(fake=True).<routine>(*args)` marshal numpy arguments into the
stand-in's SEXPs as an R caller would pass them, .Call the registered routine and marshal the result back, so that
`refpin.replay(rcall, rec)` works unchanged.  Test infrastructure only.

Arguments become SEXPs by the reference's own signatures (tests/golden/call_signatures.json): IntegerVector ->
INTSXP, NumericVector -> REALSXP, LogicalVector -> LGLSXP (logicals are int32 in the records, like integers: only the
signature tells them apart), *Matrix the same with a dim attribute and column-major data, bool / int / double a
vector of length one.  float32 arrays travel as the INTSXP bit patterns of float32@Data.  None is R_NilValue.
Arguments that are one Python object are one SEXP.
Results: a named list is a dict, a vector a numpy array by its SEXP type (LGLSXP and INTSXP both int32), a matrix
comes back in Fortran order with its dim, an INTSXP result of a float32 routine as float32, a scalar of a routine that
returns bool / int / double as that.  A result element whose SEXP IS an argument SEXP comes back as the live numpy
argument itself.  In-place changes are copied back into the live arrays.  Rf_error raises RError with its message.
`retype=True` passes each argument the way R callers also do: an integer vector as double, an int scalar as double,
a logical (vector or scalar) as integer; values convert exactly both ways.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

NILSXP, CHARSXP, LGLSXP, INTSXP, REALSXP, STRSXP, VECSXP = 0, 9, 10, 13, 14, 16, 19
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:                       # matrixextra_amd, for the real library's loader
    sys.path.insert(0, os.path.dirname(HERE))
BUILD = os.path.join(HERE, "_build")
PATHS = {False: os.path.join(BUILD, "libmxgpu_rshim.so"), True: os.path.join(BUILD, "libmxgpu_rshim_fake.so")}
PREFIX = "_MatrixExtra_"

with open(os.path.join(HERE, "golden", "call_signatures.json")) as _f:
    SIGNATURES = json.load(_f)
# the two routines of the shim that the reference does not have: `values` is a double or logical vector, or NULL
OWN_SIGNATURES = {
    "mxgpu_csr_transpose": {"arity": 4, "args": ["IntegerVector", "IntegerVector", "values", "int"], "ret": "List"},
    "mxgpu_coo_to_csr": {"arity": 5, "args": ["IntegerVector", "IntegerVector", "values", "int", "int"], "ret": "List"},
}
SXP_OF = {"IntegerVector": INTSXP, "IntegerMatrix": INTSXP, "NumericVector": REALSXP, "NumericMatrix": REALSXP,
          "LogicalVector": LGLSXP, "LogicalMatrix": LGLSXP, "bool": LGLSXP, "int": INTSXP, "double": REALSXP}
NP_OF = {LGLSXP: np.int32, INTSXP: np.int32, REALSXP: np.float64}
RETYPED = {"IntegerVector": REALSXP, "int": REALSXP, "LogicalVector": INTSXP, "LogicalMatrix": INTSXP, "bool": INTSXP}


class RError(RuntimeError):
    """Rf_error inside the shim; the text is R's message."""


def signature(name):
    return OWN_SIGNATURES.get(name) or SIGNATURES[name]


def returns_float32(name):
    ret = signature(name)["ret"]
    return ret == "IntegerMatrix" or (ret == "IntegerVector" and name.endswith("_float32"))


class Shim:
    def __init__(self, fake=False):
        path = PATHS[bool(fake)]
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C matrixextra_amd/csrc rshim`")
        if not fake:
            from matrixextra_amd import _lib
            _lib.load()
        self.fake = bool(fake)
        self.__name__ = "rcall"
        self.lib = lib = C.CDLL(path)
        for fn, res, args in (
                ("rstub_nil", C.c_void_p, ()), ("rstub_new", C.c_void_p, (C.c_int, C.c_long)),
                ("rstub_new_string", C.c_void_p, (C.c_char_p,)),
                ("rstub_data", C.c_void_p, (C.c_void_p,)), ("rstub_len", C.c_long, (C.c_void_p,)),
                ("rstub_type", C.c_int, (C.c_void_p,)), ("rstub_dead", C.c_int, (C.c_void_p,)),
                ("rstub_set_dim", None, (C.c_void_p, C.c_int, C.c_int)),
                ("rstub_dim", C.c_int, (C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int))),
                ("rstub_names", C.c_char_p, (C.c_void_p, C.c_long)), ("rstub_elt", C.c_void_p, (C.c_void_p, C.c_long)),
                ("rstub_string", C.c_char_p, (C.c_void_p, C.c_long)),
                ("rstub_call", C.c_int, (C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p))),
                ("rstub_error_message", C.c_char_p, ()), ("rstub_protect_depth", C.c_int, ()),
                ("rstub_precious_count", C.c_int, ()), ("rstub_violations", C.c_int, (C.c_char_p, C.c_int)),
                ("rstub_clear_violations", None, ()), ("rstub_torture", None, (C.c_int,)),
                ("rstub_object_count", C.c_int, ()), ("rstub_fail_allocation", None, (C.c_int,)),
                ("rstub_allocations", C.c_int, ()), ("rstub_dynamic_symbols", C.c_int, ()), ("rstub_reset", None, ()),
                ("rstub_registered", C.c_int, (C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int))),
                ("R_init_mxgpu_r", None, (C.c_void_p,))):
            f = getattr(lib, fn)
            f.restype, f.argtypes = res, args
        lib.R_init_mxgpu_r(None)
        self.nil = lib.rstub_nil()
        self.registered = []                    # (name, address, arity) in table order
        k = 0
        name, fn, n = C.c_char_p(), C.c_void_p(), C.c_int()
        while lib.rstub_registered(k, C.byref(name), C.byref(fn), C.byref(n)):
            self.registered.append((name.value.decode(), fn.value, n.value))
            k += 1
        self.routines = {nm[len(PREFIX):] if nm.startswith(PREFIX) else nm: (addr, n) for nm, addr, n in self.registered}
        self.last = None                        # what the last call passed and got, for the tests to look at

    # ------------------------------------------------------------------ the stand-in's state
    def torture(self, on):
        self.lib.rstub_torture(int(bool(on)))

    def reset(self):
        self.lib.rstub_reset()
        self.last = None

    def violations(self):
        buf = C.create_string_buffer(1 << 16)
        n = self.lib.rstub_violations(buf, len(buf))
        return n, buf.value.decode()

    def assert_clean(self, what=""):
        """after a call: the protect stack is where it was (empty), nothing is left on the precious list, no violation"""
        n, log = self.violations()
        assert n == 0, f"{what}: the R stand-in logged {n} violation(s):\n{log}"
        assert self.lib.rstub_protect_depth() == 0, f"{what}: protect stack left at depth {self.lib.rstub_protect_depth()}"
        assert self.lib.rstub_precious_count() == 0, f"{what}: {self.lib.rstub_precious_count()} object(s) left on the precious list"

    # ------------------------------------------------------------------ numpy -> SEXP
    def vector(self, sxp, data, dim=None):
        data = np.ascontiguousarray(data, dtype=NP_OF[sxp]).reshape(-1)
        s = self.lib.rstub_new(sxp, data.size)
        if data.size:
            C.memmove(self.lib.rstub_data(s), data.ctypes.data, data.nbytes)
        if dim is not None:
            self.lib.rstub_set_dim(s, int(dim[0]), int(dim[1]))
        return s

    def to_sexp(self, value, rtype, retype=False):
        if value is None:
            return self.nil
        if rtype == "values":
            rtype = "NumericVector" if np.asarray(value).dtype == np.float64 else "LogicalVector"
            retype = False
        if rtype not in SXP_OF:
            raise TypeError(f"no SEXP mapping for an argument of Rcpp type {rtype}")
        sxp = SXP_OF[rtype]
        if isinstance(value, np.ndarray):
            dim = value.shape if value.ndim == 2 else None
            flat = value.reshape(-1, order="F")
            if value.dtype == np.float32:                      # float32@Data: the bit patterns in an integer vector
                assert sxp == INTSXP, f"a float32 array for an argument of Rcpp type {rtype}"
                return self.vector(INTSXP, np.ascontiguousarray(flat).view(np.int32), dim)
            want = np.float64 if sxp == REALSXP else np.int32
            assert value.dtype == want, f"a {value.dtype} array for an argument of Rcpp type {rtype}"
            if retype and rtype in RETYPED:
                return self.vector(RETYPED[rtype], self._converted(flat, RETYPED[rtype]), dim)
            return self.vector(sxp, flat, dim)
        assert rtype in ("bool", "int", "double"), f"a scalar for an argument of Rcpp type {rtype}"
        one = np.array([value], dtype=NP_OF[sxp])
        if retype and rtype in RETYPED:
            return self.vector(RETYPED[rtype], self._converted(one, RETYPED[rtype]))
        return self.vector(sxp, one)

    @staticmethod
    def _converted(a, sxp):
        if sxp == INTSXP:                                      # logical as integer: the same numbers, NA stays NA
            return a
        out = a.astype(np.float64)                             # integer as double: NA_integer_ is NA_real_
        out[a == np.int32(-2147483648)] = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
        return out

    # ------------------------------------------------------------------ SEXP -> numpy
    def read_vector(self, s):
        sxp, n = self.lib.rstub_type(s), self.lib.rstub_len(s)
        out = np.empty(n, dtype=NP_OF[sxp])
        if n:
            C.memmove(out.ctypes.data, self.lib.rstub_data(s), out.nbytes)
        return out

    def describe(self, s):
        """SEXP types of a result: a dict by element name for a list, else the type"""
        sxp = self.lib.rstub_type(s)
        if sxp != VECSXP:
            return sxp
        out = {}
        for k in range(self.lib.rstub_len(s)):
            nm = self.lib.rstub_names(s, k)
            out[nm.decode() if nm is not None else k] = self.lib.rstub_type(self.lib.rstub_elt(s, k))
        return out

    def from_sexp(self, s, name, owners):
        lib = self.lib
        if s in owners:
            return owners[s]
        sxp = lib.rstub_type(s)
        if sxp == NILSXP:
            return None
        if sxp == VECSXP:
            out = {}
            for k in range(lib.rstub_len(s)):
                nm = lib.rstub_names(s, k)
                out[nm.decode() if nm is not None else k] = self.from_sexp(lib.rstub_elt(s, k), None, owners)
            return out
        if sxp == STRSXP:
            strings = [lib.rstub_string(s, k).decode() for k in range(lib.rstub_len(s))]
            return strings[0] if len(strings) == 1 else strings
        v = self.read_vector(s)
        if name is not None:
            ret = signature(name)["ret"]
            if ret in ("bool", "int", "double") and v.size == 1:
                return {"bool": bool, "int": int, "double": float}[ret](v[0])
            if sxp == INTSXP and returns_float32(name):
                v = v.view(np.float32)
        nr, nc = C.c_int(), C.c_int()
        if lib.rstub_dim(s, C.byref(nr), C.byref(nc)):
            v = v.reshape((nr.value, nc.value), order="F")
        return v

    # ------------------------------------------------------------------ .Call
    def call(self, name, args, retype=False, as_types=None):
        """`as_types`: argument position -> SEXP type, for passing that one argument as a vector of another type"""
        if name not in self.routines:
            raise AttributeError(f"the shim registers no routine {name}")
        addr, arity = self.routines[name]
        sig = signature(name)
        args = list(args)
        if name == "reverse_columns_inplace_binary" and len(args) == 3:       # (p, j, ncol): the values vector is empty
            args.insert(2, np.zeros(0))
        assert len(args) == arity == sig["arity"], f"{name}: {len(args)} arguments for arity {arity}"
        sexps, owners, made = [], {}, {}
        for k, (a, t) in enumerate(zip(args, sig["args"])):
            if isinstance(a, np.ndarray) and id(a) in made:
                sexps.append(made[id(a)])
                continue
            if as_types and k in as_types:
                with np.errstate(invalid="ignore"):
                    s = self.vector(as_types[k], np.asarray(a).reshape(-1, order="F").astype(NP_OF[as_types[k]]))
            else:
                s = self.to_sexp(a, t, retype)
            if isinstance(a, np.ndarray):
                made[id(a)] = s
                owners.setdefault(s, a)
            sexps.append(s)
        before = [None if s == self.nil else self.read_vector(s).tobytes() for s in sexps]
        types = [self.lib.rstub_type(s) for s in sexps]
        arr = (C.c_void_p * arity)(*sexps)
        out = C.c_void_p()
        status = self.lib.rstub_call(C.c_void_p(addr), arity, arr, C.byref(out))
        self.last = dict(name=name, sexps=sexps, types=types, before=before, result=out.value, status=status)
        for s, a in owners.items():                            # in-place routines write the caller's vectors
            now = self.read_vector(s)
            if a.dtype == np.float32:
                now = now.view(np.float32)
            if now.dtype == a.dtype and now.size == a.size and a.flags.writeable:
                a.reshape(-1, order="F")[...] = now
        if status != 0:
            raise RError(self.lib.rstub_error_message().decode("utf-8", "replace"))
        return self.from_sexp(out.value, name, owners)

    def symbol(self, name):
        """address of an exported symbol of the library"""
        return C.cast(getattr(self.lib, name), C.c_void_p).value

    def raw_call(self, addr, sexps):
        """.Call of an address with ready SEXPs: (status, result SEXP)"""
        arr = (C.c_void_p * max(len(sexps), 1))(*sexps)
        out = C.c_void_p()
        status = self.lib.rstub_call(C.c_void_p(addr), len(sexps), arr, C.byref(out))
        return status, out.value

    def error_message(self):
        return self.lib.rstub_error_message().decode("utf-8", "replace")

    def arguments_after(self):
        """bytes of every argument SEXP after the last call, beside self.last['before']"""
        return [None if s == self.nil else self.read_vector(s).tobytes() for s in self.last["sexps"]]

    def __getattr__(self, name):
        if name.startswith("_") or name in ("routines", "lib", "registered"):
            raise AttributeError(name)
        if name not in self.routines:
            raise AttributeError(f"the shim registers no routine {name}")
        return lambda *args, **kw: self.call(name, args, **kw)


_loaded = {}


def load(fake=False):
    if fake not in _loaded:
        _loaded[fake] = Shim(fake)
    return _loaded[fake]


def __getattr__(name):                                          # module level: the shim over the real libmxgpu.so
    if name.startswith("__"):
        raise AttributeError(name)
    return getattr(load(False), name)

