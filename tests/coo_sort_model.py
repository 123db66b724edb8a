"""Model, fixture access and bars of the COO sort (sort_coo_indices_*, src/misc.cpp:387-457).  Test infrastructure only.

The reference argsorts the triplets by (indices1, indices2) with std::sort, which is not stable, and permutes all
three arrays.  Where every cell occurs once that fixes every output bit.  Where a cell repeats, the index arrays are
still fixed, and so is the multiset of values of each cell, but not their order: the device keeps input order (a
stable sort), which is one of the orders the reference may give, and the numpy model below does the same.

Bars (all exact; the routine only moves data): index arrays bit for bit; values bit for bit (f64 as uint64, so NaN
payloads and the sign of zero count) for unique cells; for repeated cells the per-cell multiset of value bits against
the reference, and the order against the stable model.
"""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coo_sort_golden.npz")
KINDS = ("numeric", "logical", "binary")
VALUE_DTYPE = {"numeric": np.float64, "logical": np.int32, "binary": None}
NA_LOGICAL = np.int32(-2147483648)


def model(i, j, x=None):
    """Sorted copies: a stable argsort by (i, j) (np.lexsort is stable), applied to all three arrays."""
    i, j = np.asarray(i, dtype=np.int32), np.asarray(j, dtype=np.int32)
    o = np.lexsort((j, i))
    return i[o], j[o], None if x is None else np.asarray(x)[o]


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def has_repeats(i, j):
    cells = np.stack([np.asarray(i), np.asarray(j)], axis=1)
    return np.unique(cells, axis=0).shape[0] != cells.shape[0]


def _sorted_within_cells(i, j, xb):
    """Value bits ordered inside each run of equal (i, j): the per-cell multisets, comparable with =="""
    return xb[np.lexsort((xb, j, i))]


def assert_matches_reference(got, ref, what):
    """got / ref: (i, j, x or None) after the sort.  Indices bit for bit; values bit for bit where cells are unique,
    else equal multisets per cell."""
    gi, gj, gx = got
    ri, rj, rx = ref
    assert gi.dtype == np.int32 and gj.dtype == np.int32, what
    assert np.array_equal(gi, ri), f"{what}: row indices differ"
    assert np.array_equal(gj, rj), f"{what}: column indices differ"
    assert (gx is None) == (rx is None), what
    if rx is None:
        return
    assert gx.dtype == rx.dtype and gx.shape == rx.shape, what
    if has_repeats(ri, rj):
        assert np.array_equal(_sorted_within_cells(gi, gj, bits(gx)), _sorted_within_cells(ri, rj, bits(rx))), \
            f"{what}: the values of some cell are not the reference's"
    else:
        assert np.array_equal(bits(gx), bits(rx)), f"{what}: values differ"


def assert_equals_model(got, inp, what):
    """got is exactly the stable sort of inp: repeated cells in input order, every bit."""
    mi, mj, mx = model(*inp)
    gi, gj, gx = got
    assert np.array_equal(gi, mi) and np.array_equal(gj, mj), f"{what}: indices differ from the stable sort"
    assert (gx is None) == (mx is None), what
    if mx is not None:
        assert gx.dtype == mx.dtype and np.array_equal(bits(gx), bits(mx)), f"{what}: values differ from the stable sort"


# ----------------------------------------------------------------------------- seeded inputs
def values_for(kind, n, rng):
    if kind == "binary":
        return None
    if kind == "logical":
        return rng.choice(np.array([0, 1, NA_LOGICAL], dtype=np.int32), size=n)
    x = rng.normal(size=n).round(3)
    if n >= 4:       # NaN payloads (R's NA_real_ among them), both zeros, an infinity
        x[:4] = np.array([0x7FF00000000007A2, 0x7FF8000000000123, 0x8000000000000000, 0x7FF0000000000000],
                         dtype=np.uint64).view(np.float64)
        x = x[rng.permutation(n)]
    return x


def unique_cells(nrow, ncol, n, rng):
    """n distinct cells of an nrow x ncol matrix, shuffled"""
    flat = rng.choice(nrow * ncol, size=n, replace=False)
    return (flat // ncol).astype(np.int32), (flat % ncol).astype(np.int32)


def repeated_cells(nrow, ncol, n, rng):
    """n entries over an nrow x ncol matrix with replacement (n well above nrow * ncol / 2: many repeats)"""
    return rng.integers(0, nrow, size=n).astype(np.int32), rng.integers(0, ncol, size=n).astype(np.int32)


# ----------------------------------------------------------------------------- the fixture
def save(records, meta, path=PATH):
    """records: dicts with kind, label, i, j, x (inputs) and ri, rj, rx (what the reference left in them)"""
    arrays, index = {}, []
    for k, r in enumerate(records):
        index.append({"kind": r["kind"], "label": r["label"]})
        for key in ("i", "j", "x", "ri", "rj", "rx"):
            if r[key] is not None:
                arrays[f"r{k}_{key}"] = r[key]
    doc = {"meta": meta, "records": index}
    np.savez_compressed(path, index=np.frombuffer(json.dumps(doc).encode(), dtype=np.uint8), **arrays)


def load(path=PATH):
    Z = np.load(path)
    doc = json.loads(Z["index"].tobytes().decode())
    records = []
    for k, e in enumerate(doc["records"]):
        r = dict(e)
        for key in ("i", "j", "x", "ri", "rj", "rx"):
            name = f"r{k}_{key}"
            r[key] = Z[name] if name in Z.files else None
        records.append(r)
    return records, doc["meta"]


def run(M, kind, i, j, x):
    """M.sort_coo_indices_<kind> on fresh copies; returns them as the call left them"""
    i, j, x = i.copy(), j.copy(), None if x is None else x.copy()
    if kind == "binary":
        M.sort_coo_indices_binary(i, j)
    else:
        getattr(M, "sort_coo_indices_" + kind)(i, j, x)
    return i, j, x
