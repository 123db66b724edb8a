"""The plain model of the CSR assignment, numpy only, and the golden file of what the reference's
own compiled set_* routines (src/assignment.cpp) return.

Model, for rows that are sorted: a row the row selector does not select comes out entry for entry; a selected row
drops the entries whose column is selected (zero route) or becomes the ascending merge of its kept entries and one
(col, value) per selected column (const route); in a row replacement the selected row i[k] becomes row k of the
value.  Values are 64-bit patterns throughout: NA_real_ and other NaNs keep their payload.
"""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assign_golden.npz")
NA_REAL = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
OTHER_NAN = np.array([0xFFF8000000001234], dtype=np.uint64).view(np.float64)[0]

# every export with the arguments that follow (indptr, indices, values), in the reference's order
ORDER = {
    "set_single_row_to_zero": ["row"],
    "set_single_col_to_zero": ["col"],
    "set_single_val_to_zero": ["row", "col"],
    "set_rowseq_to_zero": ["rst", "rend"],
    "set_colseq_to_zero": ["cst", "cend", "ncols"],
    "set_arbitrary_rows_to_zero": ["rows"],
    "set_arbitrary_cols_to_zero": ["cols", "ncols"],
    "set_arbitrary_rows_single_col_to_zero": ["rows", "col", "ncols"],
    "set_single_row_arbitrary_cols_to_zero": ["row", "cols", "ncols"],
    "set_arbitrary_rows_arbitrary_cols_to_zero": ["rows", "cols", "ncols"],
    "set_single_row_to_const": ["ncols", "row", "val"],
    "set_single_col_to_const": ["ncols", "col", "val"],
    "set_single_val_to_const": ["ncols", "row", "col", "val"],
    "set_rowseq_to_const": ["rst", "rend", "ncols", "val"],
    "set_colseq_to_const": ["cst", "cend", "ncols", "val"],
    "set_arbitrary_rows_to_const": ["rows", "ncols", "val"],
    "set_arbitrary_cols_to_const": ["cols", "ncols", "val"],
    "set_arbitrary_rows_single_col_to_const": ["rows", "col", "val", "ncols"],
    "set_single_row_arbitrary_cols_to_const": ["row", "cols", "ncols", "val"],
    "set_arbitrary_rows_arbitrary_cols_to_const": ["rows", "cols", "ncols", "val"],
    "set_rowseq_to_smat": ["rst", "rend", "vp", "vj", "vx"],
    "set_arbitrary_rows_to_smat": ["rows", "vp", "vj", "vx"],
}
SCALAR_EXPORTS = [n for n in ORDER if not n.endswith("_smat")]
# the two scalar exports that always build new vectors (src/assignment.cpp:1135-1171, :1293-1364)
NEVER_ALIAS = ("set_rowseq_to_zero", "set_colseq_to_const")
ARRAY_ARGS = ("rows", "cols", "vp", "vj", "vx")
SCALAR_ARGS = ("row", "col", "rst", "rend", "cst", "cend", "ncols", "val")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def is_zero_route(value):
    """R/assignment.R:121: !is.na(value) && value == 0 (-0.0 included)."""
    return bool(value == 0)


def selectors(args):
    """(rows, cols) of a record's arguments as 0-based int arrays, None for all."""
    rows = cols = None
    if "row" in args:
        rows = np.array([args["row"]])
    elif "rst" in args:
        rows = np.arange(args["rst"], args["rend"] + 1)
    elif "rows" in args:
        rows = np.asarray(args["rows"])
    if "col" in args:
        cols = np.array([args["col"]])
    elif "cst" in args:
        cols = np.arange(args["cst"], args["cend"] + 1)
    elif "cols" in args:
        cols = np.asarray(args["cols"])
    return rows, cols


def sort_rows(p, j, x):
    """Sorted copies of (indices, values), row by row (stable)."""
    j, x = np.array(j, dtype=np.int32), np.array(x, dtype=np.float64)
    for r in range(len(p) - 1):
        s, e = p[r], p[r + 1]
        o = np.argsort(j[s:e], kind="stable")
        j[s:e], x[s:e] = j[s:e][o], x[s:e][o]
    return j, x


def assign_scalar(p, j, x, ncols, rows, cols, value):
    """(indptr, indices, values) of X[rows, cols] <- value; rows / cols None for all.  `ncols` is only read on the
    const route with all columns."""
    p, j, xb = np.asarray(p), np.asarray(j), bits(x)
    nrows = len(p) - 1
    row_sel = np.ones(nrows, dtype=bool) if rows is None else np.isin(np.arange(nrows), rows)
    zero = is_zero_route(value)
    if cols is None:
        cols_sorted = None if zero else np.arange(ncols, dtype=np.int32)
    else:
        cols_sorted = np.sort(np.asarray(cols, dtype=np.int32))
    vb = bits(np.array([value]))[0]
    out_p, out_j, out_x = [0], [], []
    for r in range(nrows):
        rj, rx = j[p[r]:p[r + 1]], xb[p[r]:p[r + 1]]
        if row_sel[r]:
            keep = np.zeros(rj.size, dtype=bool) if cols is None else ~np.isin(rj, cols_sorted)
            rj, rx = rj[keep], rx[keep]
            if not zero:
                mj = np.concatenate([rj, cols_sorted])
                mx = np.concatenate([rx, np.full(cols_sorted.size, vb, dtype=np.uint64)])
                o = np.argsort(mj, kind="stable")
                rj, rx = mj[o], mx[o]
        out_j.append(rj)
        out_x.append(rx)
        out_p.append(out_p[-1] + rj.size)
    return (np.array(out_p, dtype=np.int32), np.concatenate(out_j).astype(np.int32) if out_j else np.zeros(0, np.int32),
            (np.concatenate(out_x) if out_x else np.zeros(0, np.uint64)).astype(np.uint64).view(np.float64))


def replace_rows(p, j, x, rows, vp, vj, vx):
    """(indptr, indices, values) of X[rows, ] <- V: row rows[k] becomes row k of V, in any order of rows."""
    p, j, xb = np.asarray(p), np.asarray(j), bits(x)
    vp, vj, vxb = np.asarray(vp), np.asarray(vj), bits(vx)
    nrows = len(p) - 1
    where = np.full(nrows, -1)
    where[np.asarray(rows)] = np.arange(len(rows))
    out_p, out_j, out_x = [0], [], []
    for r in range(nrows):
        k = where[r]
        if k >= 0:
            rj, rx = vj[vp[k]:vp[k + 1]], vxb[vp[k]:vp[k + 1]]
        else:
            rj, rx = j[p[r]:p[r + 1]], xb[p[r]:p[r + 1]]
        out_j.append(rj)
        out_x.append(rx)
        out_p.append(out_p[-1] + rj.size)
    return (np.array(out_p, dtype=np.int32), np.concatenate(out_j).astype(np.int32) if out_j else np.zeros(0, np.int32),
            (np.concatenate(out_x) if out_x else np.zeros(0, np.uint64)).astype(np.uint64).view(np.float64))


def run(name, p, j, x, args):
    """The model's result of export `name` on the record's arguments."""
    rows, cols = selectors(args)
    if name.endswith("_smat"):
        return replace_rows(p, j, x, rows, args["vp"], args["vj"], args["vx"])
    value = 0.0 if name.endswith("_to_zero") else args["val"]
    return assign_scalar(p, j, x, args.get("ncols"), rows, cols, value)


def alias_rule(name, p, out_p, nnz_in):
    """Which vectors of the result are the input vectors themselves, export by export:
    (indptr, indices, values) as 0 / 1."""
    if name.endswith("_smat") or name in NEVER_ALIAS:
        return (0, 0, 0)
    if out_p[-1] != nnz_in:
        return (0, 0, 0)
    # same number of entries: the zero route removed nothing, the const route had every selected cell stored
    return (1, 1, 1) if name.endswith("_to_zero") else (1, 1, 0)


def call_args(name, args):
    """The positional arguments after (indptr, indices, values), fresh copies of the arrays."""
    return [np.array(args[a]) if a in ARRAY_ARGS else args[a] for a in ORDER[name]]


# ---- the golden file -------------------------------------------------------------------------------------------------
# Two pools hold every array of every record (one int32, one of f64 bit patterns); a record names (offset, length)
# spans in them, and equal arrays share a span (the few input matrices are stored once).
_INT_KEYS = ("p", "j", "out_p", "out_j", "rows", "cols", "vp", "vj")
_F64_KEYS = ("x", "out_x", "vx", "val")


class _Pool:
    def __init__(self, dtype):
        self.dtype, self.parts, self.size, self.seen = dtype, [], 0, {}

    def put(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        a = a.view(np.uint64) if a.dtype == np.float64 else a.astype(self.dtype)
        key = a.tobytes()
        if key not in self.seen:
            self.seen[key] = (self.size, a.size)
            self.parts.append(a)
            self.size += a.size
        return list(self.seen[key])

    def array(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=self.dtype)


def save(records, meta, path=PATH):
    """records: dicts with name, label, sorted (rows of the input sorted), p, j, x, args, out_p, out_j, out_x, alias"""
    ints, f64s, index = _Pool(np.int32), _Pool(np.uint64), []
    for r in records:
        fields = {k: r[k] for k in ("p", "j", "x", "out_p", "out_j", "out_x")}
        fields.update({a: r["args"][a] for a in ARRAY_ARGS + ("val",) if a in r["args"]})
        spans = {k: (ints if k in _INT_KEYS else f64s).put(np.asarray(v, dtype=None if k in _INT_KEYS else np.float64))
                 for k, v in fields.items()}
        scal = {a: int(r["args"][a]) for a in SCALAR_ARGS if a in r["args"] and a != "val"}
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
        r = dict(name=e["name"], label=e["label"], sorted=e["sorted"], alias=tuple(e["alias"]), args=dict(e["scalars"]))
        for k, (off, n) in e["spans"].items():
            a = (ints if k in _INT_KEYS else f64s)[off:off + n].copy()
            if k == "val":
                r["args"]["val"] = a[0]
            elif k in ARRAY_ARGS:
                r["args"][k] = a
            else:
                r[k] = a
        records.append(r)
    return records, doc["meta"]
