"""The plain model of the vector-valued CSR assignment, numpy only, and the golden file of what the
reference's own compiled set_single_{row,col}_to_{rowvec,colvec,svec} routines (src/assignment.cpp:771-1133) return.

A pattern is (ii, xx, length): 0-based positions ii inside [0, length) with their values; a dense vector is the
pattern ii = 0..length-1, zeros included.  It is recycled n / length times along the axis of n entries, repetition t
shifting ii by t * length.  Values are 64-bit patterns throughout: NA_real_ and other NaNs keep their payload.

Row routes: the row becomes exactly the recycled pattern, in the order ii is given; every other row is copied entry
for entry.  Column routes, row r with q = r % length: when the pattern stores q with value v, a row that stores the
column keeps its entries with that one value replaced and a row that does not gets (col, v) at its ascending place;
when the pattern does not store q the row loses its entry of the column, if it has one.
"""
import json
import os

import numpy as np

from assign_model import NA_REAL, OTHER_NAN, _Pool, bits, sort_rows  # noqa: F401  (re-exported for the tests)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assign_vec_golden.npz")

# every export with the arguments that follow (indptr, indices, values), in the reference's order
ORDER = {
    "set_single_row_to_rowvec": ["ncols", "row", "vec"],
    "set_single_col_to_colvec": ["ncols", "col", "vec"],
    "set_single_row_to_svec": ["ncols", "row", "ii", "xx", "length"],
    "set_single_col_to_svec": ["ncols", "col", "ii", "xx", "length"],
}
ARRAY_ARGS = ("vec", "ii", "xx")
SCALAR_ARGS = ("ncols", "row", "col", "length")


def pattern_of(args):
    """(ii, xx bits, length) of a record's arguments"""
    if "vec" in args:
        v = bits(args["vec"])
        return np.arange(v.size, dtype=np.int64), v, int(v.size)
    return np.asarray(args["ii"], dtype=np.int64), bits(args["xx"]), int(args["length"])


def recycled(ii, xb, length, n):
    """the pattern along an axis of n entries: (positions, value bits)"""
    reps = n // length
    if ii.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64)
    return (np.concatenate([ii + t * length for t in range(reps)]), np.tile(xb, reps))


def _pack(out_p, out_j, out_x):
    return (np.array(out_p, dtype=np.int32),
            np.concatenate(out_j).astype(np.int32) if out_j else np.zeros(0, np.int32),
            (np.concatenate(out_x) if out_x else np.zeros(0, np.uint64)).astype(np.uint64).view(np.float64))


def assign_row(p, j, x, ncols, row, ii, xb, length):
    """(indptr, indices, values) of X[row, ] <- pattern"""
    p, j, v = np.asarray(p), np.asarray(j), bits(x)
    rj, rx = recycled(ii, xb, length, ncols)
    out_p, out_j, out_x = [0], [], []
    for r in range(len(p) - 1):
        a, b = (rj, rx) if r == row else (j[p[r]:p[r + 1]], v[p[r]:p[r + 1]])
        out_j.append(a)
        out_x.append(b)
        out_p.append(out_p[-1] + len(a))
    return _pack(out_p, out_j, out_x)


def assign_col(p, j, x, col, ii, xb, length):
    """(indptr, indices, values) of X[, col] <- pattern; rows sorted, ii ascending"""
    p, j, v = np.asarray(p), np.asarray(j), bits(x)
    where = {int(q): k for k, q in enumerate(ii)}
    out_p, out_j, out_x = [0], [], []
    for r in range(len(p) - 1):
        rj, rx = j[p[r]:p[r + 1]].copy(), v[p[r]:p[r + 1]].copy()
        hit = np.flatnonzero(rj == col)
        k = where.get(r % length)
        if k is not None:
            if hit.size:
                rx[hit[0]] = xb[k]
            else:
                at = int(np.searchsorted(rj, col))
                rj, rx = np.insert(rj, at, col), np.insert(rx, at, xb[k])
        elif hit.size:
            rj, rx = np.delete(rj, hit[0]), np.delete(rx, hit[0])
        out_j.append(rj)
        out_x.append(rx)
        out_p.append(out_p[-1] + rj.size)
    return _pack(out_p, out_j, out_x)


def run(name, p, j, x, args):
    """The model's result of export `name` on the record's arguments."""
    ii, xb, length = pattern_of(args)
    if "row" in args:
        return assign_row(p, j, x, args["ncols"], args["row"], ii, xb, length)
    return assign_col(p, j, x, args["col"], ii, xb, length)


def alias_rule(name, p, j, args):
    """Which vectors of the result are the input vectors themselves, (indptr, indices, values) as 0 / 1: the input
    structure with new values when the row already spells the recycled pattern element for element (row routes) or
    every row already stores the column (dense column route); set_single_col_to_svec never aliases."""
    p, j = np.asarray(p), np.asarray(j)
    ii, xb, length = pattern_of(args)
    if "row" in args:
        rj, _ = recycled(ii, xb, length, args["ncols"])
        r = args["row"]
        same = rj.size > 0 and np.array_equal(j[p[r]:p[r + 1]], rj)
        return (1, 1, 0) if same else (0, 0, 0)
    if name == "set_single_col_to_svec":
        return (0, 0, 0)
    every = all((j[p[r]:p[r + 1]] == args["col"]).any() for r in range(len(p) - 1))
    return (1, 1, 0) if every and len(p) > 1 else (0, 0, 0)


def call_args(name, args):
    """The positional arguments after (indptr, indices, values), fresh copies of the arrays."""
    return [np.array(args[a]) if a in ARRAY_ARGS else args[a] for a in ORDER[name]]


# ---- the golden file -------------------------------------------------------------------------------------------------
# assign_model's layout: one int32 pool and one pool of f64 bit patterns; a record names (offset, length) spans.
_INT_KEYS = ("p", "j", "out_p", "out_j", "ii")
_F64_KEYS = ("x", "out_x", "vec", "xx")


def save(records, meta, path=PATH):
    """records: dicts with name, label, sorted (rows of the input sorted), p, j, x, args, out_p, out_j, out_x, alias"""
    ints, f64s, index = _Pool(np.int32), _Pool(np.uint64), []
    for r in records:
        fields = {k: r[k] for k in ("p", "j", "x", "out_p", "out_j", "out_x")}
        fields.update({a: r["args"][a] for a in ARRAY_ARGS if a in r["args"]})
        spans = {k: (ints if k in _INT_KEYS else f64s).put(np.asarray(v, dtype=None if k in _INT_KEYS else np.float64))
                 for k, v in fields.items()}
        scal = {a: int(r["args"][a]) for a in SCALAR_ARGS if a in r["args"]}
        index.append({"name": r["name"], "label": r["label"], "sorted": bool(r["sorted"]),
                      "alias": [int(a) for a in r["alias"]], "scalars": scal, "spans": spans})
    doc = {"meta": meta, "records": index}
    np.savez_compressed(path, index=np.frombuffer(json.dumps(doc, separators=(",", ":")).encode(), dtype=np.uint8),
                        ints=ints.array(), f64_bits=f64s.array())


def load(path=PATH):
    Z = np.load(path)
    doc = json.loads(Z["index"].tobytes().decode())
    ints, f64s = Z["ints"], Z["f64_bits"].view(np.float64)
    records = []
    for e in doc["records"]:
        r = dict(name=e["name"], label=e["label"], sorted=e["sorted"], alias=tuple(e["alias"]),
                 args=dict(e["scalars"]))
        for k, (off, n) in e["spans"].items():
            a = (ints if k in _INT_KEYS else f64s)[off:off + n].copy()
            if k in ARRAY_ARGS:
                r["args"][k] = a
            else:
                r[k] = a
        records.append(r)
    return records, doc["meta"]
