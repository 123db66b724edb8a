"""A numpy model of what finishes `[`: inject_NAs_inplace_coo_*, extract_single_val_csr_*, repeat_indices_n_times
(DESIGN.md §4.18), and of inject_NAs / drop_slice on dense matrices (R/slice.R:145-236).  Written from the layout the
design states, not from the device code; tests/golden/make_na_slice_golden.py checks every record of the reference's
own compiled routines against it before writing tests/golden/na_slice_golden.npz, which this module also reads."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "na_slice_golden.npz")
NA_INT = np.int32(-2147483648)
NA_REAL_BITS = np.uint64(0x7FF00000000007A2)
NA_REAL = np.frombuffer(NA_REAL_BITS.tobytes(), dtype=np.float64)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def remainder_lines(n, na):
    """The first n - len(na) entries of what the reference's swap loop leaves of 0 .. n-1 (add_rows_cols_NA): `na`
    from its last entry down, move_to from n - 1 down, swapping positions move_to and na[ix]."""
    arr = list(range(n))
    move_to = n - 1
    for v in reversed([int(t) for t in na]):
        arr[move_to], arr[v] = v, arr[move_to]
        move_to -= 1
    return np.array(arr[:n - len(na)], dtype=np.int32)


def inject_coo(ii, jj, xx, rows_na, cols_na, nrow, ncol):
    """(ii, jj, xx) after the injection; xx float64 (NA_real_) or int32 (NA_LOGICAL)."""
    ii, jj = np.asarray(ii, dtype=np.int32), np.asarray(jj, dtype=np.int32)
    xx = np.asarray(xx)
    rows_na, cols_na = np.asarray(rows_na, dtype=np.int32), np.asarray(cols_na, dtype=np.int32)
    in_r, in_c = np.isin(ii, rows_na), np.isin(jj, cols_na)
    if rows_na.size and cols_na.size:
        drop = in_r & in_c                              # both must hold: a triplet of an NA row alone stays
    elif rows_na.size:
        drop = in_r
    else:
        drop = in_c
    keep = ~drop
    if rows_na.size > cols_na.size:
        a = np.repeat(rows_na, ncol)
        b = np.tile(np.arange(ncol, dtype=np.int32), rows_na.size)
        rem = remainder_lines(nrow, rows_na)
        oi = np.concatenate([a, np.tile(rem, cols_na.size)])
        oj = np.concatenate([b, np.repeat(cols_na, rem.size)])
    else:
        a = np.repeat(cols_na, nrow)
        b = np.tile(np.arange(nrow, dtype=np.int32), cols_na.size)
        rem = remainder_lines(ncol, cols_na)
        oj = np.concatenate([a, np.tile(rem, rows_na.size)])
        oi = np.concatenate([b, np.repeat(rows_na, rem.size)])
    if xx.dtype == np.float64:
        fill = np.full(oi.size, NA_REAL_BITS, dtype=np.uint64).view(np.float64)
    else:
        fill = np.full(oi.size, NA_INT, dtype=np.int32)
    return (np.concatenate([ii[keep], oi]).astype(np.int32), np.concatenate([jj[keep], oj]).astype(np.int32),
            np.concatenate([xx[keep], fill]))


def extract_single_val_csr(indptr, indices, values, row, col):
    """(found, value): the first entry of the row, in storage order, at the column; value None without values."""
    for k in range(int(indptr[row]), int(indptr[row + 1])):
        if indices[k] == col:
            return True, (None if values is None else values[k])
    return False, None


def repeat_indices(indices, remainder, ix_length, desired_length):
    full = int(desired_length) // int(ix_length)
    ix = np.asarray(indices, dtype=np.int64)
    parts = [ix + ix_length * rep for rep in range(full)] + [np.asarray(remainder, dtype=np.int64) + ix_length * full]
    return np.concatenate(parts).astype(np.int32)


def sliced_dense(D, i_base1, j_base1):
    """What `x[i, j]` holds as a dense matrix, NA selectors included: i_base1 / j_base1 are 1-based int arrays with
    NA_INT for an NA (None = all).  An NA line is nan throughout (inject_NAs, R/slice.R:145-208)."""
    D = np.asarray(D, dtype=np.float64)

    def axis(sel, n):
        if sel is None:
            return np.arange(n), np.zeros(n, dtype=bool)
        sel = np.asarray(sel, dtype=np.int64)
        na = sel == int(NA_INT)
        good = sel[~na]
        return np.where(na, good[0] if good.size else 1, sel) - 1, na
    ri, rna = axis(i_base1, D.shape[0])
    ci, cna = axis(j_base1, D.shape[1])
    out = D[ri][:, ci].copy()
    out[rna, :] = np.nan
    out[:, cna] = np.nan
    return out


def dropped(M, drop=True):
    """drop_slice's as.vector() on a dense result: a vector for one row or one column, else the matrix."""
    M = np.asarray(M)
    if drop and (M.shape[0] == 1 or M.shape[1] == 1):
        return M.reshape(-1)
    return M


# ---- tests/golden/na_slice_golden.npz: an index (JSON) over one int32 pool and one pool of float64 bits -------------
_F64_KEYS = ("xx_f64", "out_xx_f64", "values_f64")


class _Pool:
    def __init__(self, dtype):
        self.dtype, self.parts, self.n = dtype, [], 0

    def put(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        a = a.view(np.uint64) if a.dtype == np.float64 else a.astype(self.dtype)
        self.parts.append(a)
        self.n += a.size
        return [self.n - a.size, int(a.size)]

    def array(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=self.dtype)


def save(records, meta, path=PATH):
    """records: dicts with `name`, `label`, int scalars under `scalars`, arrays under `arrays` (a key in _F64_KEYS is
    float64, kept as bits; every other one int32) and, for a scalar result, `result_bits` (uint64)."""
    ints, f64s, index = _Pool(np.int32), _Pool(np.uint64), []
    for r in records:
        spans = {k: (f64s if k in _F64_KEYS else ints).put(v) for k, v in r["arrays"].items()}
        e = {"name": r["name"], "label": r["label"], "scalars": {k: int(v) for k, v in r["scalars"].items()},
             "spans": spans}
        if "result_bits" in r:
            e["result_bits"] = int(r["result_bits"])
        index.append(e)
    doc = {"meta": meta, "records": index}
    np.savez_compressed(path, index=np.frombuffer(json.dumps(doc, separators=(",", ":")).encode(), dtype=np.uint8),
                        ints=ints.array(), f64_bits=f64s.array())


def load(path=PATH):
    Z = np.load(path)
    doc = json.loads(Z["index"].tobytes().decode())
    ints, f64s = Z["ints"], Z["f64_bits"].view(np.float64)
    records = []
    for e in doc["records"]:
        r = dict(name=e["name"], label=e["label"], scalars=e["scalars"], arrays={})
        if "result_bits" in e:
            r["result_bits"] = np.uint64(e["result_bits"])
        for k, (off, n) in e["spans"].items():
            r["arrays"][k] = (f64s if k in _F64_KEYS else ints)[off:off + n].copy()
        records.append(r)
    return records, doc["meta"]


def model_of(r):
    """What the model gives for a golden record: (ii, jj, xx), a uint64 of the scalar's bits, or an int32 array."""
    A, S = r["arrays"], r["scalars"]
    name = r["name"]
    if name.startswith("inject_NAs_inplace_coo"):
        xx = A["xx_f64"] if name.endswith("numeric") else A["xx"]
        return inject_coo(A["ii"], A["jj"], xx, A["rows_na"], A["cols_na"], S["nrows"], S["ncols"])
    if name.startswith("extract_single_val_csr"):
        vals = A.get("values_f64") if name.endswith("numeric") else A.get("values")
        hit, v = extract_single_val_csr(A["indptr"], A["indices"], vals, S["row"], S["col"])
        return scalar_bits(name, (v if vals is not None else 1) if hit else 0)
    return repeat_indices(A["indices"], A["remainder"], S["ix_length"], S["desired_length"])


def scalar_bits(name, v):
    """the bits of an extract_single_val_csr_* result: a double, or for _logical the int it returns"""
    if name.endswith("logical"):
        return np.uint64(np.int64(int(v)).astype(np.uint64))
    return np.array([v], dtype=np.float64).view(np.uint64)[0]
