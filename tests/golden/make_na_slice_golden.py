#!/usr/bin/env python3
"""Generates tests/golden/na_slice_golden.npz: seeded inputs and what the REFERENCE's own compiled
inject_NAs_inplace_coo_{numeric,logical} (src/slice_coo.cpp:708-946), extract_single_val_csr_{numeric,logical,binary}
(src/slice.cpp:661-785) and repeat_indices_n_times (:636-659) return for them, through oracle/_ref/libmxref.so
(oracle.ref; `make -C oracle ref`).  The file holds data only: inputs, outputs, the seed and the compile flags.
Every record is checked against tests/na_slice_model.py before anything is written, bit for bit, and none is left out.
Run from the repo root:  python tests/golden/make_na_slice_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import na_slice_model as NM  # noqa: E402
from oracle import ref as Ref  # noqa: E402

SEED = 41800
DIMS = (1, 31, 32, 33, 64, 65)
NNZ = (0, 1, 63, 64, 65)
OTHER_NAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype=np.float64)[0]


def pick(rng, n, k):
    """k ascending distinct indices of [0, n)"""
    return np.sort(rng.choice(n, size=max(0, min(k, n)), replace=False)).astype(np.int32)


def with_edges(a, n):
    return np.unique(np.concatenate([a, [0, n - 1]])).astype(np.int32)


# (label, rows_na, cols_na) for an nrow x ncol matrix; a whole axis is NA in the last three
def selectors(rng, nrow, ncol):
    none = np.zeros(0, dtype=np.int32)
    yield "rows>cols", with_edges(pick(rng, nrow, 5), nrow), pick(rng, ncol, 2) if ncol > 1 or nrow > 1 else none
    yield "rows=cols", pick(rng, nrow, 3), pick(rng, ncol, min(3, nrow))
    yield "rows<cols", pick(rng, nrow, 2) if nrow > 1 or ncol > 1 else none, with_edges(pick(rng, ncol, 5), ncol)
    yield "rows only", with_edges(pick(rng, nrow, 4), nrow), none
    yield "cols only", none, with_edges(pick(rng, ncol, 4), ncol)
    yield "edges", np.unique([0, nrow - 1]).astype(np.int32), np.unique([0, ncol - 1]).astype(np.int32)
    if max(nrow, ncol) <= 33 or (nrow, ncol) == (64, 65):
        yield "all rows", np.arange(nrow, dtype=np.int32), pick(rng, ncol, 2)
        yield "all cols", pick(rng, nrow, 2), np.arange(ncol, dtype=np.int32)
        yield "all both", np.arange(nrow, dtype=np.int32), np.arange(ncol, dtype=np.int32)


def same(got, want):
    return all(np.array_equal(NM.bits(g) if g.dtype == np.float64 else g, NM.bits(w) if w.dtype == np.float64 else w)
               and g.dtype == w.dtype for g, w in zip(got, want))


def main():
    if not Ref.available():
        Ref.build()
    rng = np.random.default_rng(SEED)
    records, turn = [], 0

    def numeric(n):
        v = np.round(rng.normal(size=n), 3)
        v[::5] = 0.0
        v[3::7] = NM.NA_REAL
        v[4::11] = OTHER_NAN
        return v

    def logical(n):
        return rng.choice(np.array([0, 1, NM.NA_INT], dtype=np.int32), size=n).astype(np.int32)

    for nrow in DIMS:
        for ncol in DIMS:
            for label, rna, cna in selectors(rng, nrow, ncol):
                nnz = NNZ[turn % len(NNZ)]
                is_lgl = turn % 2 == 1
                turn += 1
                ii = rng.integers(0, nrow, size=nnz).astype(np.int32)
                jj = rng.integers(0, ncol, size=nnz).astype(np.int32)
                if nnz > 3 and rna.size and cna.size:          # entries on NA lines: both, the row alone, the column
                    ii[0], jj[0] = rna[0], cna[-1]
                    ii[1], jj[1] = rna[-1], (cna[0] + 1) % ncol
                    ii[2], jj[2] = (rna[0] + 1) % nrow, cna[0]
                if nnz > 8:
                    ii[-1], jj[-1] = ii[0], jj[0]                  # a duplicate triplet
                name = "inject_NAs_inplace_coo_" + ("logical" if is_lgl else "numeric")
                xx = logical(nnz) if is_lgl else numeric(nnz)
                if rna.size == 0 and cna.size == 0:
                    continue                                       # a 1 x 1 matrix has no smaller list to give
                out = getattr(Ref, name)(ii, jj, xx, rna, cna, nrow, ncol)
                got = (out["ii"], out["jj"], out["xx"])
                assert same(got, NM.inject_coo(ii, jj, xx, rna, cna, nrow, ncol)), f"{name} {nrow}x{ncol} {label}"
                key, okey = ("xx", "out_xx") if is_lgl else ("xx_f64", "out_xx_f64")
                records.append(dict(name=name, label=f"{nrow}x{ncol}:nnz{nnz}:{label}",
                                    scalars=dict(nrows=nrow, ncols=ncol),
                                    arrays={"ii": ii, "jj": jj, key: xx, "rows_na": rna, "cols_na": cna,
                                            "out_ii": got[0], "out_jj": got[1], okey: got[2]}))
    # the issue's example: rem is not ascending
    assert np.array_equal(NM.remainder_lines(4, [0, 3]), [2, 1])

    # extract_single_val_csr_*: rows in storage order with a repeated column (the first wins), an empty row, misses
    p = np.array([0, 5, 5, 9, 10], dtype=np.int32)
    j = np.array([7, 2, 7, 0, 2, 3, 3, 1, 3, 70], dtype=np.int32)
    xd = np.array([1.5, -2.0, 9.0, NM.NA_REAL, 4.0, 0.0, 6.0, OTHER_NAN, 8.0, -0.0])
    xl = np.array([1, 0, NM.NA_INT, 1, 1, NM.NA_INT, 1, 0, 0, 1], dtype=np.int32)
    cells = [(0, 7), (0, 2), (0, 0), (0, 5), (1, 0), (1, 7), (2, 3), (2, 1), (2, 2), (3, 70), (3, 0), (0, 70)]
    for row, col in cells:
        for kind, vals, key in (("numeric", xd, "values_f64"), ("logical", xl, "values"), ("binary", None, None)):
            name = "extract_single_val_csr_" + kind
            got = getattr(Ref, name)(p, j, row, col) if vals is None else getattr(Ref, name)(p, j, vals, row, col)
            r = dict(name=name, label=f"({row},{col})", scalars=dict(row=row, col=col),
                     arrays={"indptr": p, "indices": j}, result_bits=NM.scalar_bits(name, got))
            if vals is not None:
                r["arrays"][key] = vals
            assert NM.model_of(r) == r["result_bits"], f"{name} ({row}, {col})"
            records.append(r)

    # repeat_indices_n_times: with and without a remainder, no indices at all, one full repeat
    for label, ix, rem, ix_length, desired in (
            ("no remainder", [1, 4, 5], [], 5, 20), ("remainder", [1, 4, 5], [1], 5, 23),
            ("remainder of two", [2, 3, 7], [2, 3], 7, 31), ("empty", [], [], 4, 13), ("one repeat", [1, 2], [], 3, 3),
            ("only a remainder", [1, 9], [1], 10, 8)):
        ix, rem = np.array(ix, dtype=np.int32), np.array(rem, dtype=np.int32)
        got = Ref.repeat_indices_n_times(ix, rem, ix_length, desired)
        r = dict(name="repeat_indices_n_times", label=label, scalars=dict(ix_length=ix_length, desired_length=desired),
                 arrays={"indices": ix, "remainder": rem, "out": got})
        assert np.array_equal(NM.model_of(r), got), label
        records.append(r)

    by_name = {}
    for r in records:
        by_name[r["name"]] = by_name.get(r["name"], 0) + 1
    NM.save(records, dict(seed=SEED, flags=Ref.compile_flags(),
                          source="src/slice_coo.cpp:708-946, src/slice.cpp:636-785"))
    print(f"{NM.PATH}: {len(records)} records {by_name}, {os.path.getsize(NM.PATH)} bytes")


if __name__ == "__main__":
    main()
