"""Record / replay of calls pinned by the reference's own compiled code (tests/golden/reference_golden.npz).

A record is one call of an entry point under the reference's name: its arguments, which of them are one object,
and what the reference returned: an array, a dict of arrays, a scalar, a string, an Rcpp::stop() message, the
arguments as the call left them (in-place routines), and which result vectors ARE argument objects.  `replay` makes
the same call on another module with the same names (oracle.oracle, oracle.ref, matrixextra_amd.exports) and
`compare` applies the bars.  Test infrastructure only.

Bars (fixed by the number formats and the reference's arithmetic, not by any output of the code under test):
  * structure, alias flags, messages, copied values and values made by one IEEE operation: bit for bit, the sign of
    zero included; NaN compared as NaN-ness, and as uint64 at the cells that multiply_csr_by_dvec_with_NAs adds
    (constants written by the reference);
  * SpMM / SpMV: bit for bit for the CPU restatement (same order of additions, no FMA on either side); the device
    keeps rtol 1e-12 (f64) and 1e-5 (f32);
  * %%: |got - ref| <= 2 (2^-64 |x1| + 3 * 2^-53 |x2|), or off by exactly one floor step (compared modulo x2) where
    x1 / x2 is within rounding of an integer, on at most 2 % of a case's cells; %/%: equal, or off by exactly 1 on
    such cells; ^: rtol 1e-13 on finite results, the special values exact.  These three are the device's bars: the
    CPU restatement is compared bit for bit (device=False).

Not reference-run: R_pow belongs to R (the reference's copy is commented out, operators.cpp:1555-1598), so every ^
value in the fixture comes from the stand-in's R_pow (oracle/refshim/refshim.cpp), written to the same table as the
oracle and the device.  For ^ the records pin operand order, recycling and the fill cells only.
"""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_golden.npz")
OPS = ("mul", "pow", "div", "mod", "idiv")

SPMM = ("tcrossprod_csr_dense_", "matmul_dense_csc_", "tcrossprod_dense_csr_", "matmul_csr_dvec_", "matmul_csr_svec_")
DVEC_OPS = ("multiply_csr_by_dvec_no_NAs_numeric", "multiply_csr_by_dvec_with_NAs")


# ----------------------------------------------------------------------------- records <-> npz
class Record:
    def __init__(self, fn, args, same, label=""):
        self.fn, self.args, self.same, self.label = fn, args, same, label
        self.out = None          # ndarray | dict | scalar | str | None
        self.alias = {}          # result key -> index of the argument it is
        self.post = {}           # argument index -> array after the call
        self.err = None

    def __repr__(self):
        return f"{self.fn}[{self.label}]"


def _same_groups(args):
    same = list(range(len(args)))
    for a in range(len(args)):
        for b in range(a):
            if isinstance(args[a], np.ndarray) and args[a] is args[b]:
                same[a] = same[b]
                break
    return same


def capture(M, fn, args, label=""):
    """Calls M.fn(*args) on copies of nothing: the arguments are used as they are, so objects shared by the caller
    stay shared.  Returns the filled Record."""
    rec = Record(fn, list(args), _same_groups(args), label)
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
    live = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
    for k, s in enumerate(rec.same):
        live[k] = live[s]
    try:
        out = call(M, fn, live)
    except Exception as e:  # noqa: BLE001 - the message is the datum
        rec.err = str(e)
        rec.args = before
        return rec
    rec.args = before
    for k, a in enumerate(live):
        if isinstance(a, np.ndarray) and a.tobytes() != before[k].tobytes():
            rec.post[k] = a.copy()
    if isinstance(out, dict):
        rec.out = {}
        for key, v in out.items():
            hit = [k for k, a in enumerate(live) if isinstance(v, np.ndarray) and v is a]
            if hit:
                rec.alias[key] = hit[0]
            rec.out[key] = v
    else:
        rec.out = out
    return rec


def save(records, meta, path=PATH):
    """One npz: every distinct array once (`p<n>`), and a JSON index of the records that refers to them."""
    pool, keys = {}, {}

    def ref(a):
        if a is None:
            return None
        if isinstance(a, (bool, int, float, str)):
            if isinstance(a, float):
                return {"f": float(a).hex() if a == a else "nan"}
            return {"s": a}
        a = np.asarray(a)
        order = "F" if (a.ndim == 2 and a.flags.f_contiguous) else "C"
        key = (a.dtype.str, a.shape, order, a.tobytes(order))
        if key not in keys:
            keys[key] = len(pool)
            pool[f"p{len(pool)}"] = a
        return {"a": keys[key]}

    index = []
    for r in records:
        e = dict(fn=r.fn, label=r.label, same=r.same, args=[ref(a) for a in r.args],
                 post={str(k): ref(a) for k, a in r.post.items()}, err=r.err, alias=r.alias)
        if isinstance(r.out, dict):
            e["dict"] = {k: ref(v) for k, v in r.out.items()}
        else:
            e["out"] = ref(r.out)
        index.append(e)
    doc = dict(meta={k: (v if isinstance(v, (int, str)) else str(v)) for k, v in meta.items()}, records=index)
    np.savez_compressed(path, index=np.frombuffer(json.dumps(doc).encode(), dtype=np.uint8), **pool)


def load(path=PATH):
    Z = np.load(path)
    doc = json.loads(Z["index"].tobytes().decode())
    cache = {}

    def get(d):
        if d is None:
            return None
        if "s" in d:
            return d["s"]
        if "f" in d:
            return float("nan") if d["f"] == "nan" else float.fromhex(d["f"])
        if d["a"] not in cache:
            cache[d["a"]] = Z[f"p{d['a']}"]
            cache[d["a"]].setflags(write=False)
        return cache[d["a"]]

    recs = []
    for e in doc["records"]:
        r = Record(e["fn"], [get(a) for a in e["args"]], e["same"], e["label"])
        r.post = {int(k): get(a) for k, a in e["post"].items()}
        r.err, r.alias = e["err"], e["alias"]
        r.out = {k: get(v) for k, v in e["dict"].items()} if "dict" in e else get(e["out"])
        recs.append(r)
    return recs, doc["meta"]


# ----------------------------------------------------------------------------- calling a module under the reference's names
def _sort_sparse(kind):
    def f(M, p, j, x=None):
        if hasattr(M, "sort_sparse_indices_inplace"):          # matrixextra_amd.exports
            return M.sort_sparse_indices_inplace(p, j, x)
        if M.__name__.endswith("oracle"):                      # oracle.oracle returns sorted copies
            js, xs = M.sort_sparse_indices(p, j, x)
            j[...] = js
            if x is not None:
                x[...] = xs
            return None
        return getattr(M, "sort_sparse_indices_" + kind)(*([p, j] if x is None else [p, j, x]))
    return f


def _reverse_columns(kind):
    def f(M, p, j, *rest):
        if M.__name__.endswith("oracle"):
            return M.reverse_columns_inplace(p, j, None if kind == "binary" else rest[0], rest[-1])
        return getattr(M, "reverse_columns_inplace_" + kind)(p, j, *rest)
    return f


def _concat(M, kinds, nrows, out_kind, *flat):
    objects = []
    for n, kind in enumerate(kinds.tolist()):
        p, j, x = flat[3 * n:3 * n + 3]
        objects.append((kind, p, j, x, int(nrows[n])))
    return M.concat_csr_batch(objects, int(out_kind))


def _concat_indptr2(M, ptr1, ptr2):
    """The device has no entry point of this name: its rbind of two matrices is a two-object concat_csr_batch, whose
    indptr is the routine's result (csrc/bind.hip, indptr_offset_kernel).  Driven here with pattern operands."""
    if hasattr(M, "concat_indptr2"):
        return M.concat_indptr2(ptr1, ptr2)
    objs = [(2, p, np.zeros(int(p[-1]), dtype=np.int32), None, p.size - 1) for p in (ptr1, ptr2)]
    return M.concat_csr_batch(objs, 2)["indptr"]


ADAPT = {"concat_indptr2": _concat_indptr2, "sort_sparse_indices_numeric": _sort_sparse("numeric"), "sort_sparse_indices_logical": _sort_sparse("logical"),
         "sort_sparse_indices_binary": _sort_sparse("binary"), "concat_csr_batch": _concat}
for _k in ("numeric", "logical", "binary"):
    ADAPT["reverse_columns_inplace_" + _k] = _reverse_columns(_k)


def has(M, fn):
    if fn in ADAPT:
        if fn in ("concat_csr_batch", "concat_indptr2"):
            return hasattr(M, "concat_csr_batch")
        return True
    try:
        getattr(M, fn)
        return True
    except AttributeError:
        return False


def call(M, fn, args):
    if fn in ADAPT:
        return ADAPT[fn](M, *args)
    return getattr(M, fn)(*args)


def replay(M, rec):
    """Calls rec.fn on M with fresh copies of the recorded arguments (shared where the record shares them).
    Returns (result or exception, live arguments)."""
    live = [a.copy() if isinstance(a, np.ndarray) else a for a in rec.args]
    for k, s in enumerate(rec.same):
        live[k] = live[s]
    try:
        return call(M, rec.fn, live), live
    except Exception as e:  # noqa: BLE001
        return e, live


# ----------------------------------------------------------------------------- bars
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def exact(got, want, what, nan_bits=None):
    """Bit for bit; NaN against NaN passes as NaN-ness unless nan_bits marks the cell."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if got.size == 0:
        return
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    if got.dtype.kind != "f":
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}"
        return
    g, w = got.reshape(-1, order="F"), want.reshape(-1, order="F")
    both_nan = np.isnan(g) & np.isnan(w)
    if nan_bits is not None:
        both_nan &= ~nan_bits
    bad = np.flatnonzero((_bits(g) != _bits(w)) & ~both_nan)
    assert bad.size == 0, (f"{what}: {bad.size} differ, first at {bad[0]}: {g[bad[0]]!r} ({_bits(g)[bad[0]]:#x}) != "
                           f"{w[bad[0]]!r} ({_bits(w)[bad[0]]:#x})")


def close(got, want, rtol, atol, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol, err_msg=what)


def dvec_op(rec):
    flags = rec.args[5:10]
    return OPS[[bool(f) for f in flags].index(True)] if any(flags) else None


def dvec_operands(rec, indptr, indices):
    """(x1, x2) of every cell of a CSR (op) recycled-vector result with the structure (indptr, indices): the vector's
    element is v[(row + col * nrows) mod length(v)] (R's recycling over the column-major matrix), X's is its stored
    value or 0."""
    p, j, x, v = (np.asarray(rec.args[k]) for k in range(4))
    lhs = bool(rec.args[10])
    m = p.size - 1
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    cols = np.asarray(indices, dtype=np.int64)
    vv = v[(rows + cols * m) % v.size]
    stored = {}
    for r in range(m):
        for k in range(p[r], p[r + 1]):
            stored.setdefault((r, int(j[k])), x[k])
    xx = np.array([stored.get((int(r), int(c)), 0.0) for r, c in zip(rows, cols)], dtype=np.float64)
    return (xx, vv) if lhs else (vv, xx)


def near_integer_quotient(x1, x2):
    with np.errstate(all="ignore"):
        q = x1 / x2
        return np.abs(q - np.rint(q)) <= 2.0 ** -50 * np.maximum(np.abs(q), 1.0)


def compare_arith(op, got, want, x1, x2, what, added=None, device=True):
    """The bars of one operation on per-cell operands.  Returns the number of floor-step cells.  Off the device
    (the CPU restatement runs the reference's own long double steps and the same libm) every operation is bit for bit."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if op in ("mul", "div") or not device:
        exact(got, want, what, nan_bits=added)
        return 0
    if added is not None and added.any():
        exact(got[added], want[added], what + " (added cells)", nan_bits=np.ones(int(added.sum()), dtype=bool))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    fin = np.isfinite(want)
    exact(got[~fin], want[~fin], what + " (special values)")
    g, w, a, b = got[fin], want[fin], x1[fin], x2[fin]
    if op == "pow":
        np.testing.assert_allclose(g, w, rtol=1e-13, atol=0, err_msg=what)
        return 0
    near = near_integer_quotient(a, b)
    if op == "idiv":
        diff = g != w
        assert np.all(np.abs(g[diff] - w[diff]) == 1.0), f"{what}: %/% differs by more than one step"
        assert np.all(near[diff]), f"{what}: %/% differs where x1/x2 is not within rounding of an integer"
        steps = int(diff.sum())
    else:
        bound = 2.0 * (2.0 ** -64 * np.abs(a) + 3.0 * 2.0 ** -53 * np.abs(b))
        d = np.abs(g - w)
        inside = d <= bound
        step = ~inside & near & (np.abs(d - np.abs(b)) <= bound)
        bad = np.flatnonzero(~inside & ~step)
        assert bad.size == 0, (f"{what}: {bad.size} cells outside the %% bound, first {a[bad[0]]!r} %% {b[bad[0]]!r}: "
                               f"{g[bad[0]]!r} != {w[bad[0]]!r} (bound {bound[bad[0]]:.3e})")
        steps = int(step.sum())
    assert steps <= 0.02 * max(g.size, 1), f"{what}: {steps} floor-step cells of {g.size} exceed 2 %"
    return steps


def _added_cells(rec, out):
    p, j = np.asarray(rec.args[0]), np.asarray(rec.args[1])
    have = set()
    for r in range(p.size - 1):
        have.update((r, int(c)) for c in j[p[r]:p[r + 1]])
    rows = np.repeat(np.arange(p.size - 1), np.diff(out["indptr"]))
    return np.array([(int(r), int(c)) not in have for r, c in zip(rows, out["indices"])], dtype=bool)


# Named exception.  When remove_zero_valued_csr_logical removes something, the reference hands its int buffer of kept
# logicals to the NumericVector constructor (misc.cpp:660-662): the result is `curr` doubles read over `curr` ints,
# so only the first half of its bytes is defined (the kept logicals, in order); the rest is whatever followed them
# in memory.  The fixture stores that defined half alone, as logicals (`defined_values`, applied by the generator).
# The device returns the kept logicals as logicals and is compared with it bit for bit; a replay of the reference
# itself is cut to its defined half in the same way before it is compared.
CSR_LOGICAL_VALUES_ARE_LOGICALS = "remove_zero_valued_csr_logical"


def defined_values(values):
    """The kept logicals of a remove_zero_valued_csr_logical result: the vector itself, or the defined half of the
    reference's reinterpreted doubles."""
    v = np.ascontiguousarray(values)
    return v.view(np.int32)[:v.size].copy() if v.dtype == np.float64 else v


# Named exception, declared in DESIGN.md 4.9.  remove_zero_valued_svec_numeric: the reference collects the kept values
# into an IntegerVector (misc.cpp:914), so a removal truncates them toward zero.  The device keeps the doubles; `ii` is
# compared as usual and `xx` against the kept input values, whose truncation must be what the reference holds.
SVEC_NUMERIC_KEEPS_DOUBLES = "remove_zero_valued_svec_numeric"


def compare_svec_numeric(rec, got, live):
    want = rec.out
    if "xx" in rec.alias:                                   # nothing removed: the inputs themselves, no truncation
        return compare(rec, got, live, device=True)
    exact(got["ii"], want["ii"], f"{rec!r}[ii]")
    ii, xx = rec.args[0], rec.args[1]
    keep = xx != 0                                          # only zeros leave, with or without na.rm
    np.testing.assert_array_equal(ii[keep], want["ii"])
    kept = xx[keep]
    exact(got["xx"], kept, f"{rec!r}[xx]")
    fin = np.isfinite(kept)
    np.testing.assert_array_equal(np.trunc(kept[fin]).astype(np.int32), want["xx"][fin])


def compare_device(rec, got, live):
    """compare() on the device, with the named exceptions that every device replay of the fixture shares"""
    if rec.fn == SVEC_NUMERIC_KEEPS_DOUBLES and rec.err is None and not isinstance(got, Exception):
        return compare_svec_numeric(rec, got, live)
    return compare(rec, got, live, device=True)


def compare(rec, got, live, device):
    """Asserts that `got` (with the live arguments after the call) is what the record holds, under the bars."""
    what = repr(rec)
    if rec.err is not None:
        assert isinstance(got, Exception), f"{what}: the reference stops with {rec.err!r}, got a result"
        assert rec.err.strip() in str(got), f"{what}: message {str(got)!r} lacks {rec.err!r}"
        return
    if isinstance(got, Exception):
        raise AssertionError(f"{what}: raised {got!r}") from got
    for k, a in enumerate(rec.args):
        if isinstance(a, np.ndarray):
            exact(live[k], rec.post.get(k, a), f"{what} argument {k} after the call")
    want = rec.out
    if want is None:
        return
    if isinstance(want, (bool, int, float, str)):
        assert type(got)(want) == got or (isinstance(want, float) and np.isnan(want) and np.isnan(got)), f"{what}: {got!r} != {want!r}"
        if isinstance(want, float) and not np.isnan(want):
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), f"{what}: {got!r} != {want!r}"
        return
    if isinstance(want, dict):
        assert isinstance(got, dict), f"{what}: expected a dict"
        for key, w in want.items():
            g = got.get(key)
            if isinstance(w, str):
                assert g == w, f"{what}[{key}]: {g!r} != {w!r}"
                continue
            if w is None or (isinstance(w, np.ndarray) and w.size == 0):
                assert g is None or np.asarray(g).size == 0, f"{what}[{key}]: expected nothing"
                continue
            assert g is not None, f"{what}: no {key!r} in the result"
            if key in rec.alias:
                assert g is live[rec.alias[key]], f"{what}[{key}]: the reference returns its argument {rec.alias[key]} itself"
            else:
                assert not any(g is a for a in live), f"{what}[{key}]: an argument object where the reference returns a new vector"
        extra = [k for k in got if k not in want and got[k] is not None and (isinstance(got[k], str) or np.asarray(got[k]).size)]
        assert not extra, f"{what}: unexpected result items {extra}"
        values_key = "values" if "values" in want else ("xx" if "xx" in want else None)
        for key, w in want.items():
            if w is None or isinstance(w, str) or w.size == 0 or key == values_key:
                continue
            exact(got[key], w, f"{what}[{key}]")
        if values_key is None or want[values_key] is None or want[values_key].size == 0:
            return
        g, w = got[values_key], want[values_key]
        if rec.fn == CSR_LOGICAL_VALUES_ARE_LOGICALS and "values" not in rec.alias:
            exact(defined_values(g), w, f"{what}[values]")
        elif rec.fn == "multiply_csr_by_dvec_with_NAs":
            x1, x2 = dvec_operands(rec, want["indptr"], want["indices"])
            compare_arith(dvec_op(rec), g, w, x1, x2, what, added=_added_cells(rec, want), device=device)
        else:
            exact(g, w, f"{what}[{values_key}]")
        return
    # a plain array
    if rec.fn.startswith(SPMM) and device:
        f32 = np.asarray(want).dtype == np.float32
        close(got, want, 1e-5 if f32 else 1e-12, 1e-5 if f32 else 1e-13, what)
    elif rec.fn == "multiply_csr_by_dvec_no_NAs_numeric":
        x1, x2 = dvec_operands(rec, rec.args[0], rec.args[1])
        compare_arith(dvec_op(rec), got, want, x1, x2, what, device=device)
    elif rec.fn == "multiply_coo_by_dense_ignore_NAs_numeric":
        ii, jj, xx, v, nrows = (np.asarray(rec.args[k]) for k in range(5))
        vv = v[(ii.astype(np.int64) + jj.astype(np.int64) * int(nrows)) % v.size]
        op = OPS[[bool(f) for f in rec.args[6:11]].index(True)]
        compare_arith(op, got, want, *((xx, vv) if rec.args[11] else (vv, xx)), what, device=device)
    else:
        exact(got, want, what)
