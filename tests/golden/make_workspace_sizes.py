#!/usr/bin/env python3
"""Generates tests/golden/workspace_sizes.json: what every mxd_*_workspace_bytes function of libmxgpu.so returns over a
grid of arguments (no device is needed: they are host arithmetic).

The record was taken ONCE, from the library built at the commit before the workspace layouts moved into one struct per
kernel family (csrc/mx_workspace.h), and is what tests/test_workspace_sizes_host.py holds every later build to: callers
allocate these bytes, so a layout may not change them.  Do not regenerate it from the code under test; a new size
function is recorded when it is added and left alone afterwards (run with its name to add only that one).
Run from the repo root:  python tests/golden/make_workspace_sizes.py [function ...]
"""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from matrixextra_amd import _lib  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
INT_MAX = 2**31 - 1
SIZES = [-1, 0, 1, 2, 3, 4, 5, 4095, 4096, 4097, 2**18, 2**18 + 1, 10**6 + 3, INT_MAX]


def grid(argtypes):
    """every combination of SIZES, 2^33 added for an int64 argument (an int one stops at INT_MAX)"""
    return itertools.product(*(SIZES + [2**33] if t is C.c_int64 else SIZES for t in argtypes))


def main(only):
    lib = _lib.load()
    names = [n for n in _lib.declared_symbols() if n.startswith("mxd_") and n.endswith("_workspace_bytes")]
    record = {}
    if only:
        with open(PATH) as f:
            record = json.load(f)
        names = [n for n in names if n in only]
    for name in names:
        argtypes = _lib.HEADER.functions[name][1]
        assert all(t in (C.c_int, C.c_int64) for t in argtypes), name
        record[name] = [list(args) + [getattr(lib, name)(*args)] for args in grid(argtypes)]
    with open(PATH, "w") as f:
        json.dump(record, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{PATH}: {len(record)} functions, {sum(map(len, record.values()))} calls, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
