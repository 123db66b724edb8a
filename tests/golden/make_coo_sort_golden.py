#!/usr/bin/env python3
"""Generates tests/golden/coo_sort_golden.npz: seeded COO triplets and what the REFERENCE's own compiled
sort_coo_indices_{numeric,logical,binary} (src/misc.cpp:387-457; oracle/ref.py over oracle/_ref/libmxref.so) leaves in
them.  The file holds data only: inputs, outputs, the seed and the compile flags.  Records with unique cells fix every
output bit; the `dup_*` records repeat cells, where the reference's order inside a cell is unspecified
(tests/coo_sort_model.py says how they are compared).
Run from the repo root:  python tests/golden/make_coo_sort_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coo_sort_model as CM  # noqa: E402
from oracle import ref as Ref  # noqa: E402

SEED = 41300
records = []


def rec(kind, label, i, j, x):
    ri, rj, rx = CM.run(Ref, kind, i, j, x)
    records.append(dict(kind=kind, label=label, i=i, j=j, x=x, ri=ri, rj=rj, rx=rx))


for n_kind, kind in enumerate(CM.KINDS):
    def rng(k):
        return np.random.default_rng(SEED + 100 * n_kind + k)
    empty = np.zeros(0, dtype=np.int32)
    rec(kind, "empty", empty, empty.copy(), CM.values_for(kind, 0, rng(0)))
    rec(kind, "one", np.array([3], dtype=np.int32), np.array([5], dtype=np.int32), CM.values_for(kind, 1, rng(1)))
    i, j = CM.unique_cells(9, 7, 40, rng(2))
    rec(kind, "small", i, j, CM.values_for(kind, 40, rng(3)))
    i, j = CM.unique_cells(300, 70000, 240, rng(4))                 # three key bytes in the columns
    rec(kind, "wide", i, j, CM.values_for(kind, 240, rng(5)))
    i, j = CM.unique_cells(70000, 3, 240, rng(6))                   # three key bytes in the rows
    rec(kind, "tall", i, j, CM.values_for(kind, 240, rng(7)))
    si, sj, sx = CM.model(i, j, CM.values_for(kind, 240, rng(8)))
    rec(kind, "sorted_already", si, sj, sx)
    i, j = CM.repeated_cells(4, 5, 60, rng(9))
    rec(kind, "dup_dense", i, j, CM.values_for(kind, 60, rng(10)))
    i, j = CM.unique_cells(30, 30, 120, rng(11))
    i[90:], j[90:] = i[:30], j[:30]                                 # a quarter of the entries repeat a cell
    o = rng(12).permutation(120)
    rec(kind, "dup_some", i[o], j[o], CM.values_for(kind, 120, rng(13)))

CM.save(records, dict(seed=SEED, flags=Ref.compile_flags(), source="sort_coo_indices_*, src/misc.cpp:387-457"))
print(f"{CM.PATH}: {len(records)} records, {os.path.getsize(CM.PATH)} bytes")
