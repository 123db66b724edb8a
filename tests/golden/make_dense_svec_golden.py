#!/usr/bin/env python3
"""Generates tests/golden/dense_svec_golden.npz: seeded calls of multiply_elemwise_dense_by_svec_{numeric,float32,
integer,logical} (src/operators.cpp:3699-4379), multiply_coo_by_dense_{numeric,integer,logical,float32} and
logicaland_coo_by_dense_logical (:721-855), and what the REFERENCE's own compiled code (oracle/ref.py over
oracle/_ref/libmxref.so) returned for them.  The file holds data only: arguments, results, the seed and the compile
flags.  Per record it asserts that no position reaches the cell that the reference writes past the matrix (deviation
1 of DESIGN.md §4.15: such input must not be run through the reference at all), that the numpy restatement of the
reference (tests/dense_svec_model.py, as_reference=True) gives the same bits, and that NaN * NaN products stay under
5 % of the case; it prints the records that carry deviations 2 and 5.
Run from the repo root, after `make -C oracle ref`:  python tests/golden/make_dense_svec_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_svec_model as M  # noqa: E402
import refpin  # noqa: E402
from oracle import ref as Ref  # noqa: E402

SEED = 41500
records, dev2, dev5 = [], [], []

# (nrows, ncols): one past the tile's edge in either direction, one column (route A wins the tie with B), one row.
# The fixture stays small; tests/test_dense_svec_model.py runs the full grid of shapes against the reference live.
SHAPES = ((65, 2), (2, 65), (63, 1), (1, 64))
BIG = (("numeric", 64, 63, 64, 1), ("integer", 130, 3, 26, 1))
# the vector's pattern by the case's running number: mostly "some", every other pattern on every route now and then
ROTATE = ("some", "ends", "some", "all", "some", "one", "some", "none")


def svec(kind, nrows, ncols, length, pattern, keep, seed, label):
    X, ii, xx = M.svec_case(kind, nrows, ncols, length, pattern, seed, x_seed=SEED + 7 * nrows + ncols)
    assert not M.overruns(nrows, ncols, ii, length), f"{label}: a position reaches cell nrows * ncols (deviation 1)"
    rec = refpin.capture(Ref, M.SVEC_FN[kind], [X, ii, xx, int(length), int(keep)], label)
    assert rec.err is None, f"{label}: {rec.err}"
    want, both = M.model(kind, X, ii, xx, length, keep, as_reference=True)
    M.compare_results(rec.out, want, both, label + " (the model of the reference)")
    named = M.int_na_tail_cells(kind, X, ii, length, keep)
    if named is not None and named.any():
        dev2.append((label, int(named.sum())))
    if M.recycles_under_keep(nrows, ncols, ii.size, length, keep):
        dev5.append(label)
    records.append(rec)


n = 0
for n_kind, kind in enumerate(M.KINDS):
    for nrows, ncols in SHAPES[:4 if kind in ("numeric", "integer") else 1]:
        for length, rt in M.lengths_for(nrows, ncols):
            for keep in (0, 1):
                pattern = ROTATE[n % len(ROTATE)]
                svec(kind, nrows, ncols, length, pattern, keep, SEED + n,
                     f"{kind}-{nrows}x{ncols}-L{length}{rt}-{pattern}-{'keep' if keep else 'ignore'}")
                n += 1
for kind in M.KINDS:                               # deviations 2 and 5 for every kind, whatever the rotation gave
    svec(kind, 65, 2, 13, "some", 1, SEED + 400, f"{kind}-65x2-L13C-some-keep")
for kind, nrows, ncols, length, keep in BIG:       # whole tiles, two row tiles, a second column tile
    svec(kind, nrows, ncols, length, "some", keep, SEED + 500 + nrows,
         f"{kind}-{nrows}x{ncols}-L{length}{M.route(nrows, ncols, length)}-some-{'keep' if keep else 'ignore'}")

# the daxpy sign rule of route C (:4005-4015) next to the direct product of route B: 0 and -1 against zero cells
for kind in M.KINDS:
    X = M.make_X(kind, 6, 3, np.random.default_rng(SEED + 900), clean=True)
    X[1, :] = 0
    X[4, :] = 0
    for length in (6, 3):
        ii, xx = np.array([1, 2, 3], dtype=np.int32), np.array([0.0, -1.0, -2.0])
        rec = refpin.capture(Ref, M.SVEC_FN[kind], [X, ii, xx, length, 0], f"{kind}-signs-L{length}")
        want, both = M.model(kind, X, ii, xx, length, False, as_reference=True)
        M.compare_results(rec.out, want, both, rec.label)
        records.append(rec)
# daxpy's early return: a value of 0 leaves +0.0 where X holds NaN / Inf (route C, f64, NAs ignored)
X = np.asfortranarray(np.array([[np.nan, 1.0], [np.inf, -2.0], [3.0, np.nan], [-np.inf, 4.0]]))
rec = refpin.capture(Ref, M.SVEC_FN["numeric"], [X, np.array([1, 2], dtype=np.int32), np.array([0.0, -1.0]), 2, 0],
                     "numeric-daxpy-zero-alpha")
assert M.bits(rec.out["values"])[0] == 0 and M.bits(rec.out["values"])[1] == 0
records.append(rec)
# a NaN value on a NaN cell: the one place where only NaN-ness is compared
X = M.make_X("numeric", 64, 2, np.random.default_rng(SEED + 901))
ii, xx = M.make_vector("all", 64, np.random.default_rng(SEED + 902))
X[0, :] = [np.nan, 1.5]
xx[0] = M.NA_REAL
xx = M.sanitise("numeric", X, ii, xx, 64, allow_both_nan=True)
_, both = M.model("numeric", X, ii, xx, 64, True)
assert 0 < both.mean() <= 0.05, both.mean()
records.append(refpin.capture(Ref, M.SVEC_FN["numeric"], [X, ii, xx, 64, 1], "numeric-both-nan"))

for kind in ("numeric", "integer", "logical", "float32", "and"):
    for nnz in (0, 1, 65, 4099):
        if nnz == 4099 and kind != "integer":          # the large case once
            continue
        X, ii, jj, xx = M.coo_case(kind, nnz, SEED + 2000 + nnz)
        rec = refpin.capture(Ref, M.COO_FN[kind], [X, ii, jj, xx], f"{kind}-nnz{nnz}")
        assert rec.err is None, rec.err
        val, both = M.coo_model(kind, X, ii, jj, xx)
        M.compare_coo([X, ii, jj, xx], M.COO_FN[kind], rec.out, dict(row=ii, col=jj, val=val), rec.label)
        assert not rec.alias, "the reference copies row and col (:763-769)"
        records.append(rec)

values = np.concatenate([r.args[2] for r in records if r.fn in M.KIND_OF_FN])
assert np.isinf(values).any() and np.isnan(values).any() and (values == 0).any() and (values == -1).any()
assert dev2 and dev5
refpin.save(records, dict(seed=SEED, flags=Ref.compile_flags(),
                          source="multiply_elemwise_dense_by_svec_*, src/operators.cpp:3699-4379; "
                                 "multiply_coo_by_dense_*, logicaland_coo_by_dense_logical, :721-855"), path=M.PATH)
print(f"{M.PATH}: {len(records)} records, {os.path.getsize(M.PATH)} bytes")
print("deviation 2 (the reference holds (double)NA_INTEGER):", ", ".join(f"{a} ({b} cells)" for a, b in dev2))
print("deviation 5 (the reference loses the vector after its first segment):", ", ".join(dev5))
