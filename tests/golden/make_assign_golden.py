#!/usr/bin/env python3
"""Generates tests/golden/assign_golden.npz: seeded CSR matrices, selectors and values, and what the REFERENCE's own
compiled set_* routines (src/assignment.cpp) return for them.  The reference's assignment.cpp, misc.cpp and
oracle/refshim/refshim.cpp are compiled with assign_ref_driver.cpp into a temporary directory, with oracle/Makefile's
REF_FLAGS; the file written holds data only: inputs, outputs, which outputs are the input vectors themselves, the
seed and the compile flags.  Nothing compiled and no text of the reference is kept.

Left out on purpose: inputs of set_arbitrary_rows_to_smat whose largest selected row is nrows - 2.  The reference
then never copies the last row and leaves indptr[nrows] at 0 (the tail test `row < nrows-1`, src/assignment.cpp:2554);
the device routine does not copy that defect and tests/test_gpu_assign.py checks such a selection against the model.
Every record with sorted rows is checked against tests/assign_model.py here, before anything is written.
Run from the repo root:  python tests/golden/make_assign_golden.py
"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assign_model as AM  # noqa: E402
from oracle.ref import REFERENCE  # noqa: E402  (where the reference's sources are; MX_REFERENCE overrides)

SEED = 51600
HERE = os.path.dirname(os.path.abspath(__file__))


def ref_flags():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        return re.search(r"^REF_FLAGS := (.*)$", f.read(), flags=re.M).group(1).split()


def build(tmp):
    shim = os.path.join(ROOT, "oracle", "refshim")
    srcs = [os.path.join(REFERENCE, "src", "assignment.cpp"), os.path.join(REFERENCE, "src", "misc.cpp"),
            os.path.join(shim, "refshim.cpp"), os.path.join(HERE, "assign_ref_driver.cpp")]
    out = os.path.join(tmp, "libassignref.so")
    subprocess.check_call(["g++", *ref_flags(), "-w", "-shared", "-I", shim, "-I", os.path.join(REFERENCE, "src"),
                           "-o", out, *srcs])
    return C.CDLL(out)


def ip(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_call(lib, name, p, j, x, args):
    p, j, x = np.array(p, dtype=np.int32), np.array(j, dtype=np.int32), np.array(x, dtype=np.float64)
    g = lambda k: int(args.get(k, 0))                                               # noqa: E731
    arr = {k: np.array(args.get(k, []), dtype=np.float64 if k == "vx" else np.int32) for k in AM.ARRAY_ARGS}
    msg = C.create_string_buffer(512)
    lib.asg_ref_call.argtypes = ([C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 8 +
                                 [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int])
    rc = lib.asg_ref_call(name.encode(), ip(p), p.size, ip(j), ip(x), j.size, g("ncols"), g("row"), g("col"),
                          g("rst"), g("rend"), g("cst"), g("cend"), ip(arr["rows"]), arr["rows"].size,
                          ip(arr["cols"]), arr["cols"].size, float(args.get("val", 0.0)), ip(arr["vp"]),
                          arr["vp"].size, ip(arr["vj"]), ip(arr["vx"]), arr["vj"].size, msg, 512)
    if rc:
        raise RuntimeError(f"{name}: {msg.value.decode()}")
    outs = []
    for k, dt in enumerate((np.int32, np.int32, np.float64)):
        a = np.empty(lib.asg_ref_len(k), dtype=dt)
        lib.asg_ref_copy(k, ip(a))
        outs.append(a)
    return outs, tuple(int(lib.asg_ref_is_input(k)) for k in range(3))


def rand_csr(rng, m, n, density, sorted_rows=True, empty_rows=()):
    mask = rng.random((m, n)) < density
    mask[list(empty_rows)] = False
    p = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
    j = np.concatenate([np.flatnonzero(r) for r in mask] or [np.zeros(0)]).astype(np.int32)
    x = np.round(rng.normal(size=j.size), 3)
    x[rng.random(j.size) < 0.1] = 0.0                              # explicit zeros are entries like any other
    if not sorted_rows:
        for r in range(m):
            o = rng.permutation(p[r + 1] - p[r])
            j[p[r]:p[r + 1]], x[p[r]:p[r + 1]] = j[p[r]:p[r + 1]][o], x[p[r]:p[r + 1]][o]
    return p, j, x


def main():
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)

        def rec(name, label, p, j, x, args, sorted_rows=True):
            args = {k: args[k] for k in AM.ORDER[name]}
            (op, oj, ox), alias = ref_call(lib, name, p, j, x, args)
            if sorted_rows:
                mp, mj, mx = AM.run(name, p, j, x, args)
                assert np.array_equal(op, mp) and np.array_equal(oj, mj) and np.array_equal(AM.bits(ox), AM.bits(mx)), \
                    f"{name} / {label}: the reference differs from the model"
                assert alias == AM.alias_rule(name, p, mp, j.size), f"{name} / {label}: alias {alias}"
            records.append(dict(name=name, label=label, sorted=sorted_rows, p=p, j=j, x=x, args=args, out_p=op,
                                out_j=oj, out_x=ox, alias=alias))

        m, n = 9, 11
        rng = np.random.default_rng(SEED)
        P, J, X = rand_csr(rng, m, n, 0.35, empty_rows=(2, 8))
        # row 4 stores every column, so that selections inside it hit the alias branches; column 6 is stored by every
        # row, column 3 by none
        dense = np.ones((m, n), dtype=bool)
        mask = np.zeros((m, n), dtype=bool)
        for r in range(m):
            mask[r, J[P[r]:P[r + 1]]] = True
        mask[4] = True
        mask[:, 6] = True
        mask[:, 3] = False
        mask[4, 3] = False
        P = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
        J = np.concatenate([np.flatnonzero(r) for r in mask]).astype(np.int32)
        X = np.round(rng.normal(size=J.size), 3)
        X[::7] = 0.0
        full = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int32)    # every cell stored
        FJ = np.tile(np.arange(n, dtype=np.int32), m)
        FX = np.round(rng.normal(size=FJ.size), 3)
        EP, EJ, EX = np.zeros(m + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)
        mats = {"mixed": (P, J, X), "full": (full, FJ, FX), "empty": (EP, EJ, EX)}
        vals = {"c": 2.5, "na": AM.NA_REAL, "nan": AM.OTHER_NAN}
        row_sets = {"arb": [7, 0, 8, 4], "arb_last": [8, 2], "arb_mid": [5, 1, 3]}
        col_sets = {"arb": [10, 0, 6, 3], "arb_nohit": [3], "arb_some": [9, 3, 2, 6, 1]}

        for mat, (p, j, x) in mats.items():
            for name in AM.SCALAR_EXPORTS:
                need = AM.ORDER[name]
                const = name.endswith("_to_const")
                cases = []
                rows_opts = ([dict(row=r) for r in (0, 2, 4, m - 1)] if "row" in need else
                             [dict(rst=a, rend=b) for a, b in ((0, 0), (2, 4), (4, 4), (6, m - 1), (0, m - 1))]
                             if "rst" in need else
                             [dict(rows=np.array(v, dtype=np.int32)) for v in row_sets.values()] if "rows" in need
                             else [dict()])
                cols_opts = ([dict(col=c) for c in (0, 3, 6, n - 1)] if "col" in need else
                             [dict(cst=a, cend=b) for a, b in ((0, 0), (3, 3), (2, 7), (6, n - 1), (0, n - 1))]
                             if "cst" in need else
                             [dict(cols=np.array(v, dtype=np.int32)) for v in col_sets.values()] if "cols" in need
                             else [dict()])
                for a, ro in enumerate(rows_opts):
                    for b, co in enumerate(cols_opts):
                        cases.append((f"{a}.{b}", {**ro, **co}))
                if mat != "mixed":
                    cases = cases[::3]                             # the structure-free matrices need fewer
                for t, (tag, sel) in enumerate(cases):
                    vkeys = list(vals) if const and t % 4 == 0 else ["c"] if const else [None]
                    for vk in vkeys:
                        args = dict(sel, ncols=n)
                        if const:
                            args["val"] = vals[vk]
                        rec(name, f"{mat}:{tag}:{vk}", p, j, x, args)

        # row replacement: seq and sorted arbitrary selections (the reference wants them sorted), values with empty rows
        for mat, (p, j, x) in mats.items():
            for lbl, (a, b) in {"first": (0, 1), "mid": (3, 5), "last": (7, m - 1), "one": (4, 4)}.items():
                vp, vj, vx = rand_csr(rng, b - a + 1, n, 0.4, empty_rows=(0,) if b > a else ())
                rec("set_rowseq_to_smat", f"{mat}:{lbl}", p, j, x, dict(rst=a, rend=b, vp=vp, vj=vj, vx=vx))
            for lbl, rows in {"to_last": [0, 2, 5, m - 1], "inner": [1, 4, 6], "first": [0]}.items():
                assert max(rows) != m - 2                          # the reference's tail defect, see above
                vp, vj, vx = rand_csr(rng, len(rows), n, 0.4, empty_rows=(1,) if len(rows) > 1 else ())
                rec("set_arbitrary_rows_to_smat", f"{mat}:{lbl}", p, j, x,
                    dict(rows=np.array(rows, dtype=np.int32), vp=vp, vj=vj, vx=vx))

        # rows that are not sorted: recorded as the reference returns them, compared after sorting the rows.
        # set_single_row_arbitrary_cols_to_const is not among them: it counts the common columns before it sorts the
        # row (src/assignment.cpp:2175-2191), so on an unsorted row its sizes are wrong.
        up, uj, ux = rand_csr(rng, m, n, 0.45, sorted_rows=False, empty_rows=(2,))
        for name in ("set_arbitrary_rows_arbitrary_cols_to_zero", "set_arbitrary_rows_arbitrary_cols_to_const",
                     "set_arbitrary_cols_to_const", "set_colseq_to_zero", "set_single_row_arbitrary_cols_to_zero",
                     "set_single_col_to_const"):
            args = dict(rows=np.array([7, 0, 8, 4], dtype=np.int32), cols=np.array([10, 0, 6, 3], dtype=np.int32),
                        row=5, col=4, cst=2, cend=7, ncols=n, val=2.5)
            rec(name, "unsorted", up, uj, ux, args, sorted_rows=False)

    flags = " ".join(ref_flags())
    AM.save(records, dict(seed=SEED, flags=flags, source="set_*, src/assignment.cpp:384-769, :1135-2598"))
    print(f"{AM.PATH}: {len(records)} records, {os.path.getsize(AM.PATH)} bytes")


if __name__ == "__main__":
    main()
