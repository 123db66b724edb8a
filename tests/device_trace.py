"""matrixextra_amd/device.py on CPU tensors over a recording fake of libmxgpu.so.

device.py only marshals: it checks operands, sizes buffers, and hands pointers and numbers to the mxd_* entry points.
With `_lib.load` and `device._stream` replaced it runs on CPU tensors, and everything it decides shows in what it
calls, with which arguments, and what it allocates.  `run_case` records exactly that:

  - one record per library call: the name and every argument: a number as it is, a pointer as null or as
    [tensor name, byte offset] (an operand of the case, "fresh#n" for the n-th torch.empty of the case, "other" for
    memory that neither names, such as a .contiguous() copy), a byref cell as its number type, a byref struct by its
    members, the stream as "stream"; the operand table of mxd_csr_rbind_batch is read back from memory;
  - every torch.empty / torch.empty_like in order, with dtype and shape;
  - what comes back: shape, dtype and storage of tensors, the numbers of a DeviceCSR, plain values, and `is` where
    the result is an operand itself.

`*_workspace_bytes` returns a fixed function of its arguments; any other call writes the case's scripted values through
its byref cells and returns 0.  Nothing here computes: values that would come out of uninitialised buffers are not
recorded (`returns=False` on a case).  tests/golden/make_device_call_trace.py writes the record,
tests/test_device_trace_host.py replays it.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from matrixextra_amd import _lib, device as D
from matrixextra_amd.device import DeviceCSR

STREAM = 0x57AEA0
_BYREF = type(C.byref(C.c_int()))
NA = -2**31


def workspace_bytes(*args) -> int:
    return 64 + 16 * (sum(int(a) for a in args) % 7)


class FakeLib:
    """Attribute lookup gives a recorder.  script: {function name: [values per call]}; the values of a call are what
    its byref cells receive, in order (for mx_* host functions: the one value it returns).  A function called more
    often than its script is long repeats the last entry."""

    def __init__(self, operands: dict, script: dict):
        self.named = []                     # (name, tensor) of the case's operands
        for name, op in operands.items():
            if isinstance(op, DeviceCSR):
                self.named += [(f"{name}.{f}", getattr(op, f)) for f in ("indptr", "indices", "values")]
            elif isinstance(op, torch.Tensor):
                self.named.append((name, op))
        self.named = [(n, t) for n, t in self.named if t is not None]
        self.operands = operands
        self.fresh, self.allocations, self.calls = [], [], []
        self.script = {k: list(v) for k, v in script.items()}
        self.seen = {}

    # ---- what a pointer points into
    def where(self, address):
        if not address:
            return "null"
        if address == STREAM:
            return "stream"
        for name, t in self.named + [(f"fresh#{k}", t) for k, t in enumerate(self.fresh)]:
            store = t.untyped_storage()
            if store.data_ptr() <= address < store.data_ptr() + max(store.nbytes(), 1):
                return [name, address - t.data_ptr()]
        return "other"

    def _struct(self, s):
        out = {}
        for field, ctype in s._fields_:
            v = getattr(s, field)
            out[field] = self.where(v) if ctype is C.c_void_p else v
        return out

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def recorder(*args):
            if name.endswith("_workspace_bytes"):
                self.calls.append({"fn": name, "args": [int(a) for a in args]})
                return workspace_bytes(*args)
            nth = self.seen.get(name, 0)
            self.seen[name] = nth + 1
            if name == "mx_last_error":
                return b"scripted failure"
            scripted = self.script.get(name)
            values = list(scripted[min(nth, len(scripted) - 1)]) if scripted else []
            if name.startswith("mx_"):          # a host function: its value is scripted
                self.calls.append({"fn": name, "args": [int(a) for a in args], "returns": values[0]})
                return values[0]
            record = {"fn": name, "args": []}
            for a in args:
                if a is None:
                    record["args"].append("null")
                elif isinstance(a, C.c_void_p):
                    record["args"].append(self.where(a.value))
                elif isinstance(a, _BYREF) and isinstance(a._obj, C.Structure):
                    record["args"].append({type(a._obj).__name__: self._struct(a._obj)})
                elif isinstance(a, _BYREF):
                    cell = a._obj                       # c_int64 is c_long here, c_longlong elsewhere: name it by width
                    record["args"].append(["cell", ("float" if cell._type_ in "fd" else "int") + str(8 * C.sizeof(cell))])
                    cell.value = values.pop(0)       # a call with more cells than scripted values is a broken case
                elif isinstance(a, (bool, int)):
                    record["args"].append(int(a))
                else:
                    raise TypeError(f"{name}: argument {a!r} is neither a number, a pointer nor a byref")
            if values:
                raise ValueError(f"{name}: {len(values)} scripted values without a cell")
            if name == "mxd_csr_rbind_batch":    # the operand table lives in memory: read it back
                items = (_lib.RbindItem * args[1]).from_address(args[0].value)
                record["table"] = [self._struct(it) for it in items]
            self.calls.append(record)
            return 0
        return recorder

    # ---- torch.empty / empty_like for the duration of a case
    def allocator(self, real):
        def empty(*args, **kwargs):
            t = real(*args, **kwargs).zero_()   # nothing fills it here: norm's .item() reads a zero, not a stray NaN
            self.fresh.append(t)                # kept alive: no address is ever used twice inside a case
            self.allocations.append({"dtype": str(t.dtype), "shape": list(t.shape)})
            return t
        return empty

    # ---- what a case returns
    def describe(self, r):
        if isinstance(r, DeviceCSR):
            d = {"DeviceCSR": {"m": r.m, "K": r.K, "nnz": r.nnz, "indptr": self.describe(r.indptr),
                               "indices": self.describe(r.indices), "values": self.describe(r.values)}}
        elif isinstance(r, torch.Tensor):
            d = {"tensor": str(r.dtype), "shape": list(r.shape), "numel": r.numel(), "strides": list(r.stride()),
                 "storage": self.where(r.data_ptr())}
        elif isinstance(r, (tuple, list)):
            return [self.describe(x) for x in r]
        else:
            return {"value": r}
        same = [name for name, op in list(self.operands.items()) + self.named if op is r]
        if same:
            d["is"] = same[0]
        return d


@contextlib.contextmanager
def faked(fake: FakeLib):
    saved = _lib.load, D._stream, torch.empty, torch.empty_like
    _lib.load = lambda: fake
    D._stream = lambda: C.c_void_p(STREAM)
    torch.empty, torch.empty_like = fake.allocator(saved[2]), fake.allocator(saved[3])
    try:
        yield
    finally:
        _lib.load, D._stream, torch.empty, torch.empty_like = saved


def run_case(case) -> dict:
    operands = case["operands"]()
    fake = FakeLib(operands, case.get("script", {}))
    with faked(fake):
        result = case["run"](operands)
    out = {"calls": fake.calls, "allocations": fake.allocations}
    if case.get("returns", True):
        out["returns"] = fake.describe(result)
    state = {n: {"_sorted": op._sorted, "_order_builds": op._order_builds}
             for n, op in operands.items() if isinstance(op, DeviceCSR)}
    if state:
        out["state"] = state
    return out


def run_refusal(case) -> dict:
    operands = case["operands"]()
    fake = FakeLib(operands, case.get("script", {}))
    try:
        with faked(fake):
            case["run"](operands)
    except Exception as e:                      # noqa: BLE001 - the type is what gets recorded
        return {"type": type(e).__name__, "message": str(e)}
    return {"type": None, "message": None}


# ---- operands ---------------------------------------------------------------------------------------------------------
def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def f64(*v):
    return torch.tensor(v, dtype=torch.float64)


def f32(*v):
    return torch.tensor(v, dtype=torch.float32)


def values(kind, n=4):
    if kind == "d":
        return torch.arange(1, n + 1, dtype=torch.float64)
    if kind == "l":
        return torch.tensor(([1, 0, NA, 1] * n)[:n], dtype=torch.int32)
    if kind == "f":
        return torch.arange(1, n + 1, dtype=torch.float32)
    return None


def csr(kind="d"):
    """3 x 4 with four entries, the middle row empty"""
    return DeviceCSR(i32(0, 2, 2, 4), i32(0, 2, 1, 3), values(kind), 3, 4, 4)


def empty_csr(kind="d"):
    x = values(kind, 0)
    return DeviceCSR(i32(0, 0, 0, 0), i32(), x, 3, 4, 0)


def square(kind="d"):
    return DeviceCSR(i32(0, 2, 3, 4), i32(0, 2, 1, 2), values(kind), 3, 3, 4)


def column(kind="d"):
    """3 x 1 with two entries"""
    return DeviceCSR(i32(0, 1, 1, 2), i32(0, 0), values(kind, 2), 3, 1, 2)


def coo(kind="d"):
    return dict(i=i32(0, 0, 2, 2), j=i32(0, 2, 1, 3), x=values(kind))


def case(name, operands, run, script=None, returns=True):
    return name, dict(operands=operands, run=run, script=script or {}, returns=returns)


def _kinds(name, make, run, script, kinds="dln"):
    return [case(f"{name}[{k}]", (lambda k=k: make(k)), run, script) for k in kinds]


def cases() -> dict:
    c = []
    # ---- CSR (op) CSR
    for op, kind in (("MX_OP_ADD", "d"), ("MX_OP_OR", "l"), ("MX_OP_AND", "n")):
        c.append(case(f"csr_elemwise[{op},{kind}]", lambda kind=kind: dict(A=csr(kind), B=csr(kind)),
                      lambda o, op=op: D.csr_elemwise(getattr(_lib, op), o["A"], o["B"]),
                      {"mxd_csr_merge_count": [[5]]}))
    c.append(case("csr_elemwise[empty]", lambda: dict(A=csr(), B=csr()),
                  lambda o: D.csr_elemwise(_lib.MX_OP_MUL, o["A"], o["B"]), {"mxd_csr_merge_count": [[0]]}))
    # ---- gather
    c += _kinds("csr_gather_rows", lambda k: dict(A=csr(k), rows=i32(2, 0)),
                lambda o: D.csr_gather_rows(o["A"], o["rows"]), {"mxd_csr_gather_count": [[3]]})
    c.append(case("csr_gather_rows[empty]", lambda: dict(A=csr(), rows=i32(1)),
                  lambda o: D.csr_gather_rows(o["A"], o["rows"]), {"mxd_csr_gather_count": [[0]]}))
    # ---- transpose, COO <-> CSR, sort
    c += _kinds("csr_transpose", lambda k: dict(A=csr(k)), lambda o: D.csr_transpose(o["A"]),
                {"mxd_csr_transpose": [[4]]})
    c.append(case("csr_transpose[merged]", lambda: dict(A=csr()), lambda o: D.csr_transpose(o["A"]),
                  {"mxd_csr_transpose": [[3]]}))
    c.append(case("csr_transpose[empty]", lambda: dict(A=empty_csr()), lambda o: D.csr_transpose(o["A"]),
                  {"mxd_csr_transpose": [[0]]}))
    c += _kinds("coo_to_csr", coo, lambda o: D.coo_to_csr(o["i"], o["j"], o["x"], 3, 4), {"mxd_coo_to_csr": [[3]]})
    c.append(case("coo_to_csr[empty]", lambda: dict(i=i32(), j=i32(), x=values("d", 0)),
                  lambda o: D.coo_to_csr(o["i"], o["j"], o["x"], 3, 4), {"mxd_coo_to_csr": [[0]]}))
    c.append(case("csr_to_coo", lambda: dict(A=csr()), lambda o: D.csr_to_coo(o["A"])))
    c.append(case("csr_to_coo[empty]", lambda: dict(A=empty_csr("n")), lambda o: D.csr_to_coo(o["A"])))
    c += _kinds("coo_sort[byrow,sorted]", coo, lambda o: D.coo_sort(o["i"], o["j"], o["x"]), {"mxd_coo_sort": [[1]]})
    c.append(case("coo_sort[bycol,unsorted]", lambda: coo("l"),
                  lambda o: D.coo_sort(o["i"], o["j"], o["x"], byrow=False), {"mxd_coo_sort": [[0]]}))
    # ---- coo_slice: every selector on each axis
    take = {"rows": lambda: i32(3, 1, 1), "cols": lambda: i32(4, 2)}
    slices = [("all", "seq", "d"), ("seq", "rev", "l"), ("rev", "map", "n"), ("map", "all", "d"), ("map", "map", "l")]

    def selector(kind, o, axis):
        return {"all": ("all",), "seq": ("seq", 1, 2), "rev": ("rev", 0, 1), "map": ("map", o.get(axis))}[kind]

    for rk, ck, kind in slices:
        def make(rk=rk, ck=ck, kind=kind):
            o = coo(kind)
            if rk == "map":
                o["rows"] = take["rows"]()
            if ck == "map":
                o["cols"] = take["cols"]()
            return o
        c.append(case(f"coo_slice[{rk},{ck},{kind}]", make,
                      lambda o, rk=rk, ck=ck: D.coo_slice(o["i"], o["j"], o["x"], 3, 4, selector(rk, o, "rows"),
                                                          selector(ck, o, "cols")),
                      {"mxd_coo_slice_count": [[2]]}))
    c.append(case("coo_slice[empty]", lambda: coo("d"),
                  lambda o: D.coo_slice(o["i"], o["j"], o["x"], 3, 4, ("all",), ("seq", 0, 0)),
                  {"mxd_coo_slice_count": [[0]]}))
    c.append(case("coo_slice[empty map]", lambda: dict(coo("n"), rows=i32()),
                  lambda o: D.coo_slice(o["i"], o["j"], o["x"], 3, 4, ("map", o["rows"]), ("all",)),
                  {"mxd_coo_slice_count": [[0]]}))
    # ---- NA injection
    for kind, k in (("d", 7), ("l", 7), ("d", 0)):
        c.append(case(f"coo_inject_na[{kind},{k}]", lambda kind=kind: dict(coo(kind), rows_na=i32(1), cols_na=i32(0, 3)),
                      lambda o: D.coo_inject_na(o["i"], o["j"], o["x"], 3, 4, o["rows_na"], o["cols_na"]),
                      {"mxd_coo_inject_na_count": [[k]]}))
    c.append(case("coo_inject_na[strided x]", lambda: dict(coo("n"), x=torch.arange(8, dtype=torch.float64)[::2],
                                                           rows_na=i32(), cols_na=i32(2)),
                  lambda o: D.coo_inject_na(o["i"], o["j"], o["x"], 3, 4, o["rows_na"], o["cols_na"]),
                  {"mxd_coo_inject_na_count": [[5]]}))
    # ---- single cell
    c.append(case("csr_single[hit,d]", lambda: dict(A=csr()), lambda o: D.csr_single(o["A"], 2, 3),
                  {"mxd_csr_single": [[3, 4.0]]}))
    c.append(case("csr_single[hit,l]", lambda: dict(A=csr("l")), lambda o: D.csr_single(o["A"], 0, 2),
                  {"mxd_csr_single": [[1, NA]]}))
    c.append(case("csr_single[hit,n]", lambda: dict(A=csr("n")), lambda o: D.csr_single(o["A"], 0, 0),
                  {"mxd_csr_single": [[0, 0]]}))
    c.append(case("csr_single[miss]", lambda: dict(A=csr()), lambda o: D.csr_single(o["A"], 1, 1),
                  {"mxd_csr_single": [[-1, 0.0]]}))
    # ---- compaction
    c.append(case("csr_remove_zeros[keeps all]", lambda: dict(A=csr()), lambda o: D.csr_remove_zeros(o["A"]),
                  {"mxd_compact_count": [[4]]}))
    c.append(case("csr_remove_zeros[drops]", lambda: dict(A=csr()), lambda o: D.csr_remove_zeros(o["A"]),
                  {"mxd_compact_count": [[2]]}))
    c.append(case("csr_remove_zeros[drops all]", lambda: dict(A=csr("l")), lambda o: D.csr_remove_zeros(o["A"]),
                  {"mxd_compact_count": [[0]]}))
    c.append(case("csr_remove_zeros[na_rm,d]", lambda: dict(A=csr()), lambda o: D.csr_remove_zeros(o["A"], True),
                  {"mxd_compact_count": [[3]]}))
    c.append(case("csr_remove_zeros[na_rm,l]", lambda: dict(A=csr("l")), lambda o: D.csr_remove_zeros(o["A"], True),
                  {"mxd_compact_count": [[3]]}))
    c.append(case("csr_remove_zeros[pattern]", lambda: dict(A=csr("n")), lambda o: D.csr_remove_zeros(o["A"])))
    c.append(case("csr_filter[int32 mask]", lambda: dict(A=csr(), mask=i32(1, 0, NA, 1)),
                  lambda o: D.csr_filter(o["A"], o["mask"]), {"mxd_compact_count": [[3]]}))
    c.append(case("csr_filter[bool mask keeps all]", lambda: dict(A=csr("l"), mask=torch.ones(4, dtype=torch.bool)),
                  lambda o: D.csr_filter(o["A"], o["mask"]), {"mxd_compact_count": [[4]]}))
    # ---- CSC * dense
    def csc_dense(dtype):
        return lambda: dict(A=csr(), D=torch.ones((4, 3), dtype=dtype))
    c.append(case("csc_by_dense[values only]", csc_dense(torch.float64),
                  lambda o: D.csc_by_dense(o["A"], o["D"], keep_na=False)))
    c.append(case("csc_by_dense[kept structure]", csc_dense(torch.float64), lambda o: D.csc_by_dense(o["A"], o["D"]),
                  {"mxd_csc_dense_na_count": [[4, 0]]}))
    c.append(case("csc_by_dense[changed structure]", csc_dense(torch.float32), lambda o: D.csc_by_dense(o["A"], o["D"]),
                  {"mxd_csc_dense_na_count": [[6, 2]]}))
    c.append(case("csc_by_dense[same count, cells outside]", csc_dense(torch.float64),
                  lambda o: D.csc_by_dense(o["A"], o["D"]), {"mxd_csc_dense_na_count": [[4, 1]]}))
    c.append(case("csc_by_dense[empty count]", csc_dense(torch.float64), lambda o: D.csc_by_dense(o["A"], o["D"]),
                  {"mxd_csc_dense_na_count": [[0, 0]]}))
    c.append(case("csc_by_dense[empty X]", lambda: dict(A=empty_csr(), D=torch.ones((4, 3), dtype=torch.float64)),
                  lambda o: D.csc_by_dense(o["A"], o["D"]), {"mxd_csc_dense_na_count": [[0, 0]]}))
    c.append(case("csc_by_dense[bool]", csc_dense(torch.bool), lambda o: D.csc_by_dense(o["A"], o["D"]),
                  {"mxd_csc_dense_na_count": [[5, 1]]}))
    c.append(case("csc_by_dense[int32]", csc_dense(torch.int32), lambda o: D.csc_by_dense(o["A"], o["D"]),
                  {"mxd_csc_dense_na_count": [[5, 1]]}))
    c.append(case("csc_by_dense[int32 logical]", csc_dense(torch.int32),
                  lambda o: D.csc_by_dense(o["A"], o["D"], keep_na=False, logical=True)))
    # ---- CSR * sparse vector
    svec = dict(vi=lambda: i32(1, 3), vx=lambda: f64(2.0, 3.0))
    c.append(case("csr_by_svec[d]", lambda: dict(A=csr(), vi=svec["vi"](), vx=svec["vx"]()),
                  lambda o: D.csr_by_svec(o["A"], o["vi"], o["vx"], 3), {"mxd_csr_by_svec_count": [[5, 1]]}))
    c.append(case("csr_by_svec[n,no NA]", lambda: dict(A=csr(), vi=svec["vi"]()),
                  lambda o: D.csr_by_svec(o["A"], o["vi"], None, 3, keep_na=False), {"mxd_csr_by_svec_count": [[2, 0]]}))
    c.append(case("csr_by_svec[empty]", lambda: dict(A=csr(), vi=i32(), vx=f64()),
                  lambda o: D.csr_by_svec(o["A"], o["vi"], o["vx"], 1), {"mxd_csr_by_svec_count": [[0, 0]]}))
    c.append(case("csr_by_svec[strided vector]", lambda: dict(A=csr(), vi=i32(1, 9, 2, 9)[::2], vx=f64(1, 9, 2, 9)[::2]),
                  lambda o: D.csr_by_svec(o["A"], o["vi"], o["vx"], 3), {"mxd_csr_by_svec_count": [[3, 0]]}))
    # ---- dense * sparse vector
    routes = {"A": _lib.MX_DSV_ROUTE_A, "B": _lib.MX_DSV_ROUTE_B, "C": _lib.MX_DSV_ROUTE_C, "D": _lib.MX_DSV_ROUTE_D}
    for route, dtype, logical, length, k in (("A", torch.float64, False, 12, None), ("D", torch.bool, False, 5, None),
                                             ("B", torch.float32, False, 3, 8), ("C", torch.int32, False, 3, 4),
                                             ("B", torch.int32, True, 3, 0)):
        c.append(case(f"dense_by_svec[route {route},{str(dtype)[6:]}{',logical' if logical else ''},{k}]",
                      lambda dtype=dtype: dict(X=torch.ones((3, 4), dtype=dtype), vi=svec["vi"](), vx=svec["vx"]()),
                      lambda o, logical=logical, length=length: D.dense_by_svec(o["X"], o["vi"], o["vx"], length,
                                                                                logical=logical),
                      {"mx_dense_by_svec_route": [[routes[route]]], "mxd_dense_by_svec_count": [[k]]}))
    c.append(case("dense_by_svec[no NA,empty vector]",
                  lambda: dict(X=torch.ones((3, 4), dtype=torch.float64), vi=i32(), vx=f64()),
                  lambda o: D.dense_by_svec(o["X"], o["vi"], o["vx"], 3, keep_na=False),
                  {"mx_dense_by_svec_route": [[routes["B"]]], "mxd_dense_by_svec_count": [[0]]}))
    # ---- CSR (op) dense vector with R's NA cells
    def dvec(n):
        return lambda: dict(A=csr(), v=torch.arange(1, n + 1, dtype=torch.float64))
    c.append(case("csr_by_dvec_keep_na[rows]", dvec(3), lambda o: D.csr_by_dvec_keep_na(o["A"], o["v"]),
                  {"mxd_csr_by_dvec_na_rows_count": [[6]]}))
    c.append(case("csr_by_dvec_keep_na[rows,empty]", dvec(1), lambda o: D.csr_by_dvec_keep_na(o["A"], o["v"], "/"),
                  {"mxd_csr_by_dvec_na_rows_count": [[0]]}))
    c.append(case("csr_by_dvec_keep_na[flat,no candidates]", dvec(5), lambda o: D.csr_by_dvec_keep_na(o["A"], o["v"], "^"),
                  {"mxd_dvec_na_special": [[0, 0]]}))
    c.append(case("csr_by_dvec_keep_na[flat,nothing new]", dvec(2), lambda o: D.csr_by_dvec_keep_na(o["A"], o["v"], "%%"),
                  {"mxd_dvec_na_special": [[1, 3]], "mxd_dvec_na_cells_count": [[0]]}))
    c.append(case("csr_by_dvec_keep_na[flat,new cells]", dvec(12), lambda o: D.csr_by_dvec_keep_na(o["A"], o["v"], "%/%"),
                  {"mxd_dvec_na_special": [[2, 5]], "mxd_dvec_na_cells_count": [[3]], "mxd_coo_to_csr": [[3]]}))
    # ---- outer products, row vector * CSC
    for name, v in (("f64", f64), ("f32", f32)):
        c.append(case(f"csr_outer_dense[{name}]", lambda v=v: dict(A=column(), v=v(1, 2, 3)),
                      lambda o: D.csr_outer_dense(o["A"], o["v"]), {"mxd_csr_outer_dense_count": [[6]]}))
    c.append(case("csr_outer_dense[empty]", lambda: dict(A=column(), v=f64()),
                  lambda o: D.csr_outer_dense(o["A"], o["v"]), {"mxd_csr_outer_dense_count": [[0]]}))
    outer = {"mxd_csr_outer_svec_count": [[2, 4]]}
    c.append(case("csr_outer_svec[d]", lambda: dict(A=column(), vi=svec["vi"](), vx=svec["vx"]()),
                  lambda o: D.csr_outer_svec(o["A"], o["vi"], o["vx"], 5), outer))
    c.append(case("csr_outer_svec[i]", lambda: dict(A=column(), vi=svec["vi"](), vx=i32(2, NA)),
                  lambda o: D.csr_outer_svec(o["A"], o["vi"], o["vx"], 5), outer))
    c.append(case("csr_outer_svec[l]", lambda: dict(A=column(), vi=svec["vi"](), vx=i32(1, NA)),
                  lambda o: D.csr_outer_svec(o["A"], o["vi"], o["vx"], 5, v_dtype=_lib.MX_LGL), outer))
    c.append(case("csr_outer_svec[n]", lambda: dict(A=column(), vi=svec["vi"]()),
                  lambda o: D.csr_outer_svec(o["A"], o["vi"], None, 5), outer))
    c.append(case("csr_outer_svec[empty]", lambda: dict(A=column(), vi=i32(), vx=f64()),
                  lambda o: D.csr_outer_svec(o["A"], o["vi"], o["vx"], 0), {"mxd_csr_outer_svec_count": [[2, 0]]}))
    c += _kinds("rowvec_by_csc", lambda k: dict(A=csr(k), v=f32(1, 2, 3, 4)), lambda o: D.rowvec_by_csc(o["v"], o["A"]),
                {}, "dn")
    # ---- rbind / cbind
    def bind_operands():
        return dict(A=csr("d"), B=csr("l"), P=csr("n"), vi=i32(1, 4), vd=f64(1, 2), vl=i32(1, NA))

    c.append(case("csr_rbind[every kind]", bind_operands,
                  lambda o: D.csr_rbind([o["A"], o["B"], o["P"], (o["vi"], o["vd"], 4), (o["vi"], o["vl"], 5, "i"),
                                         (o["vi"], o["vl"], 4), (o["vi"], None, 6), (o["vi"], o["vd"], 4, "d"),
                                         (o["vi"], o["vl"], 4, "l"), (o["vi"], o["vl"], 4, "n")])))
    c.append(case("csr_rbind[logical]", bind_operands,
                  lambda o: D.csr_rbind(iter([(o["vi"], None, 4, "n"), o["B"], o["P"]]))))
    c.append(case("csr_rbind[pattern]", bind_operands, lambda o: D.csr_rbind([o["P"], (o["vi"], None, 7)])))
    c.append(case("csr_rbind[integer vector]", bind_operands, lambda o: D.csr_rbind([o["P"], (o["vi"], o["vl"], 4, "i")])))
    c += _kinds("csr_cbind", lambda k: dict(A=csr(k), B=square(k)), lambda o: D.csr_cbind(o["A"], o["B"]), {})
    for kind, vx, vkind, first in (("d", "vd", None, False), ("n", None, None, True), ("l", "vl", None, False),
                                   ("n", "vl", "i", True), ("l", "vd", "n", False), ("n", "vl", "l", False)):
        c.append(case(f"csr_cbind_svec[{kind},{vx},{vkind},first={first}]",
                      lambda kind=kind: dict(bind_operands(), A=csr(kind)),
                      lambda o, vx=vx, vkind=vkind, first=first: D.csr_cbind_svec(o["A"], o["vi"], o.get(vx), 5, first,
                                                                                  vkind)))
    # ---- reductions
    for na_rm in (False, True):
        c.append(case(f"segment_reduce[na_rm={na_rm}]",
                      lambda: dict(x=values("l"), segptr=i32(0, 1, 4), perm=i32(3, 2, 1, 0)),
                      lambda o, na_rm=na_rm: D.segment_reduce(o["x"], "sq_sum", o["segptr"], 4, o["perm"], na_rm)))
        c.append(case(f"row_reduce[na_rm={na_rm}]", lambda: dict(A=csr()),
                      lambda o, na_rm=na_rm: D.row_reduce(o["A"], "abs_max", na_rm)))
        c.append(case(f"col_reduce[na_rm={na_rm}]", lambda: dict(A=csr("n")),
                      lambda o, na_rm=na_rm: D.col_reduce(o["A"], na_rm=na_rm)))
    c.append(case("segment_reduce[no segments, given dtype]", lambda: dict(x=values("l"), segptr=i32(0)),
                  lambda o: D.segment_reduce(o["x"], "sum", o["segptr"], 0, value_dtype=_lib.MX_I32)))
    c.append(case("col_reduce[passed order]", lambda: dict(A=csr(), perm=i32(0, 2, 1, 3), colptr=i32(0, 1, 2, 3, 4)),
                  lambda o: D.col_reduce(o["A"], "abs_sum", order=(o["perm"], o["colptr"]))))
    c.append(case("col_reduce[twice: one order]", lambda: dict(A=csr()),
                  lambda o: (D.col_reduce(o["A"]), D.col_reduce(o["A"], "sq_sum"))))
    for kind, type in (("d", "O"), ("l", "I"), ("d", "F"), ("n", "M")):
        c.append(case(f"norm[{type},{kind}]", lambda kind=kind: dict(A=csr(kind)),
                      lambda o, type=type: D.norm(o["A"], type), returns=False))
    c.append(case("norm[no entries]", lambda: dict(A=empty_csr()), lambda o: D.norm(o["A"], "F")))
    c.append(case("norm[no columns]", lambda: dict(A=DeviceCSR(i32(0, 0), i32(), None, 1, 0, 0)),
                  lambda o: D.norm(o["A"], "M")))
    for kind, flag in (("d", 1), ("l", 0), ("n", 1)):
        c.append(case(f"diag[{kind}]", lambda kind=kind: dict(A=csr(kind)), lambda o: D.diag(o["A"]),
                      {"mxd_csr_rows_sorted": [[flag]]}))
    c.append(case("diag[sortedness known]", lambda: dict(A=DeviceCSR(i32(0, 1, 2), i32(0, 1), f64(1, 2), 2, 2, 2, True)),
                  lambda o: D.diag(o["A"])))
    # ---- cached properties of a DeviceCSR
    for flag in (0, 1):
        c.append(case(f"rows_sorted[{flag},twice]", lambda: dict(A=csr()),
                      lambda o: (o["A"].rows_sorted(), o["A"].rows_sorted()), {"mxd_csr_rows_sorted": [[flag]]}))
    c.append(case("column_order[twice]", lambda: dict(A=csr()),
                  lambda o: (lambda first, second: (first, second, first is second))(o["A"].column_order(),
                                                                                   o["A"].column_order())))
    c.append(case("column_order[empty]", lambda: dict(A=empty_csr("n")), lambda o: o["A"].column_order()))
    # ---- structured operands
    c.append(case("csr_triangle_check", lambda: dict(A=square()),
                  lambda o: (D.csr_triangle_check(o["A"], "U"), D.csr_triangle_check(o["A"], "L", strict=True)),
                  {"mxd_csr_triangle_check": [[0], [2]]}))
    c += _kinds("csr_symmetric_to_general", lambda k: dict(A=square(k)), lambda o: D.csr_symmetric_to_general(o["A"], "U"),
                {"mxd_csr_symmetric_to_general_count": [[6]]})
    c.append(case("csr_symmetric_to_general[empty]", lambda: dict(A=DeviceCSR(i32(0, 0, 0), i32(), f64(), 2, 2, 0)),
                  lambda o: D.csr_symmetric_to_general(o["A"], "L"), {"mxd_csr_symmetric_to_general_count": [[0]]}))
    c.append(case("csr_symmetric_count", lambda: dict(A=square()), lambda o: D.csr_symmetric_count(o["A"], "L"),
                  {"mxd_csr_symmetric_to_general_count": [[5]]}))

    def fill_into(o, with_x):
        out_p, ws, k = D.csr_symmetric_count(o["A"], "U")
        return D.csr_symmetric_fill(o["A"], "U", out_p, ws, k, o["out_j"], o["out_x"] if with_x else None)

    c.append(case("csr_symmetric_fill[given buffers]",
                  lambda: dict(A=square(), out_j=torch.zeros(8, dtype=torch.int32),
                               out_x=torch.zeros(8, dtype=torch.float64)),
                  lambda o: fill_into(o, True), {"mxd_csr_symmetric_to_general_count": [[6]]}))
    c.append(case("csr_symmetric_fill[given indices only]",
                  lambda: dict(A=square("l"), out_j=torch.zeros(8, dtype=torch.int32), out_x=None),
                  lambda o: fill_into(o, False), {"mxd_csr_symmetric_to_general_count": [[6]]}))
    c += _kinds("csr_unit_triangular_to_general", lambda k: dict(A=square(k)),
                lambda o: D.csr_unit_triangular_to_general(o["A"], "L"), {})
    c.append(case("csr_unit_triangular_to_general[given buffers]",
                  lambda: dict(A=square(), p=torch.zeros(4, dtype=torch.int32), j=torch.zeros(9, dtype=torch.int32),
                               x=torch.zeros(9, dtype=torch.float64)),
                  lambda o: D.csr_unit_triangular_to_general(o["A"], "U", (o["p"], o["j"], o["x"]))))
    c.append(case("csr_unit_triangular_to_general[0 x 0]", lambda: dict(A=DeviceCSR(i32(0), i32(), None, 0, 0, 0)),
                  lambda o: D.csr_unit_triangular_to_general(o["A"], "U")))
    out = dict(c)
    assert len(out) == len(c), "two cases share a name"
    return out


def refusals() -> dict:
    """One case per `raise` of the functions in scope: the exception's type and its full message."""
    big = 2**31 - 1
    strided = i32(0, 9, 0, 9, 2, 9, 2, 9)[::2]
    r = []
    r.append(case("_value_dtype", lambda: coo("f"), lambda o: D.coo_to_csr(o["i"], o["j"], o["x"], 3, 4)))
    r.append(case("csr_transpose: values", lambda: dict(A=csr("f")), lambda o: D.csr_transpose(o["A"])))
    r.append(case("csr_gather_rows: values", lambda: dict(A=csr("f"), rows=i32(0)),
                  lambda o: D.csr_gather_rows(o["A"], o["rows"]), {"mxd_csr_gather_count": [[2]]}))
    for fn, call in (("coo_to_csr", lambda o: D.coo_to_csr(o["i"], o["j"], o["x"], 3, 4)),
                     ("coo_sort", lambda o: D.coo_sort(o["i"], o["j"], o["x"])),
                     ("coo_slice", lambda o: D.coo_slice(o["i"], o["j"], o["x"], 3, 4, ("all",), ("all",))),
                     ("coo_inject_na", lambda o: D.coo_inject_na(o["i"], o["j"], o["x"], 3, 4, i32(), i32()))):
        r.append(case(f"{fn}: j shorter", lambda: dict(coo(), j=i32(0, 2, 1)), call))
        r.append(case(f"{fn}: x longer", lambda: dict(coo(), x=values("d", 5)), call))
        if fn != "coo_slice":
            r.append(case(f"{fn}: int64 i", lambda: dict(coo(), i=torch.tensor([0, 0, 2, 2])), call))
            r.append(case(f"{fn}: strided j", lambda: dict(coo(), j=strided), call))
    r.append(case("coo_sort: strided x", lambda: dict(coo(), x=torch.arange(8, dtype=torch.float64)[::2]),
                  lambda o: D.coo_sort(o["i"], o["j"], o["x"])))
    r.append(case("coo_sort: float32 x", lambda: coo("f"), lambda o: D.coo_sort(o["i"], o["j"], o["x"])))
    r.append(case("coo_slice: float32 x", lambda: coo("f"),
                  lambda o: D.coo_slice(o["i"], o["j"], o["x"], 3, 4, ("all",), ("all",))))
    r.append(case("coo_inject_na: no x", lambda: coo("n"),
                  lambda o: D.coo_inject_na(o["i"], o["j"], o["x"], 3, 4, i32(), i32())))
    r.append(case("coo_inject_na: int64 rows_na", lambda: coo(),
                  lambda o: D.coo_inject_na(o["i"], o["j"], o["x"], 3, 4, torch.tensor([1]), i32())))
    r.append(case("coo_inject_na: float32 x", lambda: coo("f"),
                  lambda o: D.coo_inject_na(o["i"], o["j"], o["x"], 3, 4, i32(), i32())))
    r.append(case("csr_single: row", lambda: dict(A=csr()), lambda o: D.csr_single(o["A"], 3, 0)))
    r.append(case("csr_single: negative row before values", lambda: dict(A=csr("f")), lambda o: D.csr_single(o["A"], -1, 0)))
    r.append(case("csr_filter: pattern", lambda: dict(A=csr("n")), lambda o: D.csr_filter(o["A"], i32(1, 1, 1, 1))))
    r.append(case("csr_filter: mask length", lambda: dict(A=csr()), lambda o: D.csr_filter(o["A"], i32(1, 1, 1))))
    r.append(case("csr_filter: mask dtype", lambda: dict(A=csr()), lambda o: D.csr_filter(o["A"], f64(1, 1, 1, 1))))
    ones = torch.ones((4, 3), dtype=torch.float64)
    r.append(case("csc_by_dense: pattern X", lambda: dict(A=csr("n")), lambda o: D.csc_by_dense(o["A"], ones)))
    r.append(case("csc_by_dense: logical X", lambda: dict(A=csr("l")), lambda o: D.csc_by_dense(o["A"], ones)))
    r.append(case("csc_by_dense: shape", lambda: dict(A=csr()), lambda o: D.csc_by_dense(o["A"], ones.t())))
    r.append(case("csc_by_dense: dtype", lambda: dict(A=csr()), lambda o: D.csc_by_dense(o["A"], ones.to(torch.int64))))
    vi, vx = i32(1, 3), f64(2, 3)
    r.append(case("csr_by_svec: X", lambda: dict(A=csr("l")), lambda o: D.csr_by_svec(o["A"], vi, vx, 3)))
    r.append(case("csr_by_svec: vi dtype", lambda: dict(A=csr()), lambda o: D.csr_by_svec(o["A"], vi.long(), vx, 3)))
    r.append(case("csr_by_svec: vi 2-d", lambda: dict(A=csr()), lambda o: D.csr_by_svec(o["A"], vi[None], vx, 3)))
    r.append(case("csr_by_svec: vx dtype", lambda: dict(A=csr()), lambda o: D.csr_by_svec(o["A"], vi, vx.float(), 3)))
    r.append(case("csr_by_svec: vx shape", lambda: dict(A=csr()), lambda o: D.csr_by_svec(o["A"], vi, f64(1), 3)))
    r.append(case("csr_by_svec: length", lambda: dict(A=csr()), lambda o: D.csr_by_svec(o["A"], vi, vx, 2)))
    r.append(case("csr_by_svec: more positions than length", lambda: dict(A=csr()),
                  lambda o: D.csr_by_svec(o["A"], vi, vx, 1)))
    X = torch.ones((3, 4), dtype=torch.float64)
    route = {"mx_dense_by_svec_route": [[_lib.MX_DSV_ROUTE_B]]}
    r.append(case("dense_by_svec: X 1-d", dict, lambda o: D.dense_by_svec(X[0], vi, vx, 3)))
    r.append(case("dense_by_svec: dtype", dict, lambda o: D.dense_by_svec(X.to(torch.int64), vi, vx, 3)))
    r.append(case("dense_by_svec: vi", dict, lambda o: D.dense_by_svec(X, vi.long(), vx, 3)))
    r.append(case("dense_by_svec: vx", dict, lambda o: D.dense_by_svec(X, vi, vx.float(), 3)))
    r.append(case("dense_by_svec: vx shape", dict, lambda o: D.dense_by_svec(X, vi, f64(1), 3)))
    r.append(case("dense_by_svec: no route", dict, lambda o: D.dense_by_svec(X, vi, vx, -1),
                  {"mx_dense_by_svec_route": [[-1]]}))
    r.append(case("dense_by_svec: more positions than length", dict, lambda o: D.dense_by_svec(X, vi, vx, 1), route))
    r.append(case("dense_by_svec: position 0", dict, lambda o: D.dense_by_svec(X, i32(0, 2), vx, 3), route))
    r.append(case("dense_by_svec: position past length", dict, lambda o: D.dense_by_svec(X, i32(1, 4), vx, 3), route))
    v = f64(1, 2, 3)
    r.append(case("csr_by_dvec_keep_na: op", lambda: dict(A=csr()), lambda o: D.csr_by_dvec_keep_na(o["A"], v, "+")))
    r.append(case("csr_by_dvec_keep_na: X", lambda: dict(A=csr("n")), lambda o: D.csr_by_dvec_keep_na(o["A"], v)))
    r.append(case("csr_by_dvec_keep_na: v dtype", lambda: dict(A=csr()), lambda o: D.csr_by_dvec_keep_na(o["A"], v.float())))
    r.append(case("csr_by_dvec_keep_na: v 2-d", lambda: dict(A=csr()), lambda o: D.csr_by_dvec_keep_na(o["A"], v[None])))
    r.append(case("csr_by_dvec_keep_na: empty v", lambda: dict(A=csr()), lambda o: D.csr_by_dvec_keep_na(o["A"], f64())))
    r.append(case("csr_by_dvec_keep_na: long v", lambda: dict(A=csr()),
                  lambda o: D.csr_by_dvec_keep_na(o["A"], torch.ones(13, dtype=torch.float64))))
    for fn, call in (("csr_outer_dense", lambda o: D.csr_outer_dense(o["A"], v)),
                     ("csr_outer_svec", lambda o: D.csr_outer_svec(o["A"], vi, vx, 5))):
        r.append(case(f"{fn}: columns", lambda: dict(A=csr()), call))
        r.append(case(f"{fn}: X", lambda: dict(A=column("l")), call))
    r.append(case("csr_outer_dense: v", lambda: dict(A=column()), lambda o: D.csr_outer_dense(o["A"], i32(1, 2))))
    r.append(case("csr_outer_svec: vi", lambda: dict(A=column()), lambda o: D.csr_outer_svec(o["A"], vi.long(), vx, 5)))
    r.append(case("csr_outer_svec: vx", lambda: dict(A=column()), lambda o: D.csr_outer_svec(o["A"], vi, vx.float(), 5)))
    r.append(case("csr_outer_svec: vx shape", lambda: dict(A=column()), lambda o: D.csr_outer_svec(o["A"], vi, i32(1), 5)))
    r.append(case("csr_outer_svec: length", lambda: dict(A=column()), lambda o: D.csr_outer_svec(o["A"], vi, vx, 1)))
    r.append(case("csr_outer_svec: negative length", lambda: dict(A=column()),
                  lambda o: D.csr_outer_svec(o["A"], i32(), None, -1)))
    r.append(case("rowvec_by_csc: v", lambda: dict(A=csr()), lambda o: D.rowvec_by_csc(f32(1, 2, 3), o["A"])))
    r.append(case("rowvec_by_csc: f64 v", lambda: dict(A=csr()), lambda o: D.rowvec_by_csc(f64(1, 2, 3, 4), o["A"])))
    r.append(case("rowvec_by_csc: Y", lambda: dict(A=csr("l")), lambda o: D.rowvec_by_csc(f32(1, 2, 3, 4), o["A"])))
    r.append(case("csr_rbind: nothing", dict, lambda o: D.csr_rbind([])))
    r.append(case("csr_rbind: int64 indices", lambda: dict(A=csr()), lambda o: D.csr_rbind([o["A"], (vi.long(), vx, 4)])))
    r.append(case("csr_rbind: strided indices", lambda: dict(A=csr()), lambda o: D.csr_rbind([(strided, None, 4)])))
    r.append(case("csr_rbind: values shorter", lambda: dict(A=csr()), lambda o: D.csr_rbind([o["A"], (vi, f64(1), 4)])))
    r.append(case("csr_rbind: float32 values", lambda: dict(A=csr("f")), lambda o: D.csr_rbind([o["A"]])))
    r.append(case("csr_rbind: rows", lambda: dict(A=DeviceCSR(i32(0), i32(), None, big, 4, 0)),
                  lambda o: D.csr_rbind([o["A"]])))
    r.append(case("csr_cbind: kinds", lambda: dict(A=csr(), B=csr("l")), lambda o: D.csr_cbind(o["A"], o["B"])))
    r.append(case("csr_cbind: columns", lambda: dict(A=csr(), B=DeviceCSR(i32(0, 0, 0, 0), i32(), f64(), 3, big, 0)),
                  lambda o: D.csr_cbind(o["A"], o["B"])))
    r.append(case("csr_cbind_svec: vi", lambda: dict(A=csr()), lambda o: D.csr_cbind_svec(o["A"], vi.long(), vx, 5)))
    r.append(case("csr_cbind_svec: vx length", lambda: dict(A=csr()), lambda o: D.csr_cbind_svec(o["A"], vi, f64(1), 5)))
    r.append(case("csr_cbind_svec: length", lambda: dict(A=csr()), lambda o: D.csr_cbind_svec(o["A"], vi, vx, 1)))
    r.append(case("csr_cbind_svec: float32 values", lambda: dict(A=csr()),
                  lambda o: D.csr_cbind_svec(o["A"], vi, vx.float(), 5)))
    r.append(case("segment_reduce: op", dict, lambda o: D.segment_reduce(vx, "mean", i32(0, 2), 2)))
    r.append(case("row_reduce: op", lambda: dict(A=csr()), lambda o: D.row_reduce(o["A"], "max")))
    r.append(case("col_reduce: order", lambda: dict(A=csr()),
                  lambda o: D.col_reduce(o["A"], order=(i32(0, 1, 2), i32(0, 1, 2, 3, 3)))))
    r.append(case("col_reduce: colptr", lambda: dict(A=csr()),
                  lambda o: D.col_reduce(o["A"], order=(i32(0, 1, 2, 3), i32(0, 1, 2, 4)))))
    r.append(case("norm: type", lambda: dict(A=csr()), lambda o: D.norm(o["A"], "2")))
    r.append(case("csr_triangle_check: uplo", lambda: dict(A=square()), lambda o: D.csr_triangle_check(o["A"], "u")))
    r.append(case("csr_symmetric_to_general: square", lambda: dict(A=csr()),
                  lambda o: D.csr_symmetric_to_general(o["A"], "U")))
    r.append(case("csr_symmetric_to_general: uplo", lambda: dict(A=square()),
                  lambda o: D.csr_symmetric_to_general(o["A"], "X")))
    r.append(case("csr_unit_triangular_to_general: square", lambda: dict(A=csr()),
                  lambda o: D.csr_unit_triangular_to_general(o["A"], "U")))
    r.append(case("csr_unit_triangular_to_general: uplo", lambda: dict(A=square()),
                  lambda o: D.csr_unit_triangular_to_general(o["A"], "")))
    out = dict(r)
    assert len(out) == len(r), "two refusals share a name"
    return out
