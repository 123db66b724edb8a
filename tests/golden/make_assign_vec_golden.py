#!/usr/bin/env python3
"""Generates tests/golden/assign_vec_golden.npz: seeded CSR matrices, rows / columns and vector values, and what the
REFERENCE's own compiled set_single_row_to_rowvec, set_single_col_to_colvec, set_single_row_to_svec and
set_single_col_to_svec (src/assignment.cpp:771-1133) return for them.  The reference's assignment.cpp, misc.cpp and
oracle/refshim/refshim.cpp are compiled with assign_vec_ref_driver.cpp into a temporary directory, with
oracle/Makefile's REF_FLAGS; the file written holds data only: inputs, outputs, which outputs are the input vectors
themselves, the seed and the compile flags.  Nothing compiled and no text of the reference is kept.

Left out on purpose, three rules:
  1. inputs of set_single_row_to_svec where the row's length is a non-zero multiple of length(ii) but differs from
     length(ii) * n_repeats.  The reference's fast path (src/assignment.cpp:939-966) is entered on the multiple alone:
     with n_repeats <= 1 it then reads ii past its end (:944-946), with n_repeats > 1 it can "match" a shorter row and
     write n_repeats * nnz values into it, over the next rows' values.  `defective()` below is that rule, and no such
     input is recorded; tests/test_assign_vec_model.py and tests/test_gpu_assign_vec.py check them against the model.
  2. an empty ii on the row route: the reference divides by zero (:939); its R caller assigns 0 instead.
  3. set_single_row_to_rowvec on a full row that is not sorted is recorded, but its alias flags are not compared: the
     reference returns the input indptr beside new indices (:800-808), for which mx_result_info has no value.  It
     is among the records of the shuffled matrix.
Every record with sorted rows is checked against tests/assign_vec_model.py here, vectors and alias flags, before
anything is written; the records of the shuffled matrix alone are compared after sorting the rows of both sides.
Run from the repo root:  python tests/golden/make_assign_vec_golden.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_vec_model as VM  # noqa: E402
from make_assign_golden import rand_csr, ref_flags  # noqa: E402
from oracle.ref import REFERENCE  # noqa: E402  (where the reference's sources are; MX_REFERENCE overrides)

SEED = 51700
HERE = os.path.dirname(os.path.abspath(__file__))
SPECIALS = [0.0, -0.0, VM.NA_REAL, VM.OTHER_NAN]


def build(tmp):
    shim = os.path.join(ROOT, "oracle", "refshim")
    srcs = [os.path.join(REFERENCE, "src", "assignment.cpp"), os.path.join(REFERENCE, "src", "misc.cpp"),
            os.path.join(shim, "refshim.cpp"), os.path.join(HERE, "assign_vec_ref_driver.cpp")]
    out = os.path.join(tmp, "libassignvecref.so")
    subprocess.check_call(["g++", *ref_flags(), "-w", "-shared", "-I", shim, "-I", os.path.join(REFERENCE, "src"),
                           "-o", out, *srcs])
    return C.CDLL(out)


def ip(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_call(lib, name, p, j, x, args):
    p, j, x = np.array(p, dtype=np.int32), np.array(j, dtype=np.int32), np.array(x, dtype=np.float64)
    ii = np.array(args.get("ii", []), dtype=np.int32)
    xx = np.array(args["vec"] if "vec" in args else args["xx"], dtype=np.float64)
    msg = C.create_string_buffer(512)
    lib.asgv_ref_call.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    rc = lib.asgv_ref_call(name.encode(), ip(p), p.size, ip(j), ip(x), j.size, int(args["ncols"]),
                           int(args["row"] if "row" in args else args["col"]), ip(ii), ii.size, ip(xx), xx.size,
                           int(args.get("length", 0)), msg, 512)
    if rc:
        raise RuntimeError(f"{name}: {msg.value.decode()}")
    outs = []
    for k, dt in enumerate((np.int32, np.int32, np.float64)):
        a = np.empty(lib.asgv_ref_len(k), dtype=dt)
        lib.asgv_ref_copy(k, ip(a))
        outs.append(a)
    return outs, tuple(int(lib.asgv_ref_is_input(k)) for k in range(3))


def defective(p, row, n_ii, ncols, length):
    """rule 1 of the docstring"""
    row_len = int(p[row + 1] - p[row])
    return row_len > 0 and row_len % n_ii == 0 and row_len != n_ii * (ncols // length)


def from_mask(mask, rng):
    P = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
    J = np.concatenate([np.flatnonzero(r) for r in mask] or [np.zeros(0)]).astype(np.int32)
    X = np.round(rng.normal(size=J.size), 3)
    X[::7] = 0.0
    return P, J, X


def main():
    records, skipped = [], [0]
    rng = np.random.default_rng(SEED)
    turn = [0]

    def vals(n):
        """n values; 0, -0.0, NA_real_ and another NaN take turns at its positions"""
        v = np.round(rng.normal(size=n), 3) + 3.0
        for k in range(0, n, 3):
            v[k] = SPECIALS[turn[0] % 4]
            turn[0] += 1
        return v

    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)

        def rec(name, label, p, j, x, args, sorted_rows=True):
            args = {k: args[k] for k in VM.ORDER[name]}
            if name == "set_single_row_to_svec":
                assert len(args["ii"]) > 0                                          # rule 2
                if defective(p, args["row"], len(args["ii"]), args["ncols"], args["length"]):
                    skipped[0] += 1                                                 # rule 1
                    return
            (op, oj, ox), alias = ref_call(lib, name, p, j, x, args)
            if sorted_rows:
                mp, mj, mx = VM.run(name, p, j, x, args)
                assert np.array_equal(op, mp) and np.array_equal(oj, mj) and np.array_equal(VM.bits(ox), VM.bits(mx)), \
                    f"{name} / {label}: the reference differs from the model"
                assert alias == VM.alias_rule(name, p, j, args), f"{name} / {label}: alias {alias}"
            records.append(dict(name=name, label=label, sorted=sorted_rows, p=p, j=j, x=x, args=args, out_p=op,
                                out_j=oj, out_x=ox, alias=alias))

        # the 9 x 11 matrices of make_assign_golden.py: rows 2 and 8 store column 6 alone, row 4 stores every column
        # but 3, column 6 is stored by every row, column 3 by none; `full` stores every cell, `empty` none
        m, n = 9, 11
        P, J, _ = rand_csr(rng, m, n, 0.35, empty_rows=(2, 8))
        mask = np.zeros((m, n), dtype=bool)
        for r in range(m):
            mask[r, J[P[r]:P[r + 1]]] = True
        mask[4] = True
        mask[:, 6] = True
        mask[:, 3] = False
        mixed = from_mask(mask, rng)
        full = from_mask(np.ones((m, n), dtype=bool), rng)
        empty = (np.zeros(m + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
        # 8 x 12, so that row lengths 12, 6, 4, 3 and column lengths 8, 4, 2 recycle: row 5 empty, row 3 full,
        # column 7 stored by every row but the empty one, column 2 by the full row alone
        mask = rng.random((8, 12)) < 0.35
        mask[5] = False
        mask[3] = True
        mask[:, 7] = True
        mask[:, 2] = False
        mask[3, 2] = True
        mask[5] = False
        wide = from_mask(mask, rng)
        # rows in random order, one of them full
        up, uj, ux = rand_csr(rng, m, n, 0.45, sorted_rows=False, empty_rows=(2,))
        umask = np.zeros((m, n), dtype=bool)
        for r in range(m):
            umask[r, uj[up[r]:up[r + 1]]] = True
        umask[4] = True
        up, uj, ux = from_mask(umask, rng)
        for r in range(m):
            o = rng.permutation(up[r + 1] - up[r])
            uj[up[r]:up[r + 1]], ux[up[r]:up[r + 1]] = uj[up[r]:up[r + 1]][o], ux[up[r]:up[r + 1]][o]
        assert not np.array_equal(uj[up[4]:up[5]], np.arange(n))

        shapes = {"mixed": (mixed, n, (0, 2, 4, m - 1), (0, 3, 6, n - 1), (11, 1), (9, 3, 1)),
                  "full": (full, n, (0, 4, m - 1), (0, 6, n - 1), (11, 1), (9, 3, 1)),
                  "empty": (empty, n, (0, m - 1), (0, n - 1), (11, 1), (9, 3, 1)),
                  "wide": (wide, 12, (0, 3, 5, 7), (0, 2, 7, 11), (12, 6, 4, 3), (8, 4, 2)),
                  "shuffled": ((up, uj, ux), n, (0, 2, 4, m - 1), (0, 5, n - 1), (11, 1), (9, 3, 1))}

        def some(length, k):
            """k ascending positions inside [0, length)"""
            return np.sort(rng.choice(length, size=min(k, length), replace=False)).astype(np.int32)

        for mat, ((p, j, x), nc, rows, cols, row_lens, col_lens) in shapes.items():
            srt = mat != "shuffled"
            nr = len(p) - 1
            for row in rows:
                for L in row_lens:
                    rec("set_single_row_to_rowvec", f"{mat}:r{row}:L{L}", p, j, x, dict(ncols=nc, row=row, vec=vals(L)),
                        srt)
                    ii = some(L, max(1, L // 3))
                    rec("set_single_row_to_svec", f"{mat}:r{row}:L{L}:sorted", p, j, x,
                        dict(ncols=nc, row=row, ii=ii, xx=vals(ii.size), length=L), srt)
                    if L > 2:
                        ii = rng.permutation(some(L, max(2, L // 2))).astype(np.int32)
                        rec("set_single_row_to_svec", f"{mat}:r{row}:L{L}:unsorted", p, j, x,
                            dict(ncols=nc, row=row, ii=ii, xx=vals(ii.size), length=L), srt)
                # an ii that is the row's own indices: the structure stays the caller's
                own = j[p[row]:p[row + 1]].astype(np.int32)
                if own.size:
                    rec("set_single_row_to_svec", f"{mat}:r{row}:own", p, j, x,
                        dict(ncols=nc, row=row, ii=own, xx=vals(own.size), length=nc), srt)
            for col in cols:
                for L in col_lens:
                    rec("set_single_col_to_colvec", f"{mat}:c{col}:L{L}", p, j, x, dict(ncols=nc, col=col, vec=vals(L)),
                        srt)
                    for tag, ii in (("some", some(L, max(1, L // 2))), ("all", np.arange(L, dtype=np.int32)),
                                    ("none", np.zeros(0, dtype=np.int32))):
                        rec("set_single_col_to_svec", f"{mat}:c{col}:L{L}:{tag}", p, j, x,
                            dict(ncols=nc, col=col, ii=ii, xx=vals(ii.size), length=L), srt)
            assert nr % max(col_lens) == 0 and nc % max(row_lens) == 0

        # the recycled alias of the row route: a row that spells a pattern of length 4 three times over
        rp = np.array([0, 2, 8, 8], dtype=np.int32)
        rj = np.array([1, 5, 0, 3, 4, 7, 8, 11], dtype=np.int32)
        rx = np.arange(1.0, 9.0)
        rec("set_single_row_to_svec", "recycled:own", rp, rj, rx,
            dict(ncols=12, row=1, ii=np.array([0, 3], dtype=np.int32), xx=vals(2), length=4))
        # the explicit zero of the issue: written into a row that stored the column
        rec("set_single_col_to_svec", "explicit zero", np.array([0, 1, 2], dtype=np.int32),
            np.array([1, 1], dtype=np.int32), np.array([1.0, 2.0]),
            dict(ncols=3, col=1, ii=np.array([0, 1], dtype=np.int32), xx=np.array([50.0, 0.0]), length=2))
        rec("set_single_row_to_rowvec", "issue example", np.array([0, 1, 2], dtype=np.int32),
            np.array([1, 0], dtype=np.int32), np.array([1.0, 2.0]),
            dict(ncols=6, row=0, vec=np.array([0.0, 7.0, VM.OTHER_NAN])))

    by_name = {k: sum(r["name"] == k for r in records) for k in VM.ORDER}
    assert all(v >= 20 for v in by_name.values()), by_name
    assert any(r["alias"] == (1, 1, 0) for r in records if r["name"] == "set_single_row_to_svec")
    n_sorted = sum(r["sorted"] for r in records)
    flags = " ".join(ref_flags())
    VM.save(records, dict(seed=SEED, flags=flags, sorted_records=n_sorted, shuffled_records=len(records) - n_sorted,
                          left_out_by_rule_1=skipped[0],
                          source="set_single_{row,col}_to_{rowvec,colvec,svec}, src/assignment.cpp:771-1133"))
    print(f"{VM.PATH}: {len(records)} records ({n_sorted} sorted, {skipped[0]} left out by rule 1) {by_name}, "
          f"{os.path.getsize(VM.PATH)} bytes")


if __name__ == "__main__":
    main()
