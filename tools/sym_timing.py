#!/usr/bin/env python3
"""Device-event timing of the symmetric and unit-triangular expansions: 5 warm-up runs, then 20
timed runs, median and min.

Input: a square n = 1,000,000 upper triangle with 16 stored entries per row (column r + 1 + k * stride, wrapped
rows dropped, so the last rows are shorter), none on the diagonal: the general form has about 32 M entries, cfg2's
count.  For the f64 and the pattern kind:

  sym_count          mxd_csr_symmetric_to_general_count: column order, row ids, row lengths, scan, one read-back
  sym_fill           mxd_csr_symmetric_to_general_fill into tensors allocated once
  unit_tri           mxd_csr_unit_triangular_to_general into tensors allocated once

Each stands next to `copy_ms`, a device-to-device copy of the bytes of the result it writes (index pointer, indices,
values), and the symmetric expansion next to what was available before this family, in the same process:

  transpose_alone    device.csr_transpose of the same triangle
  transpose_merge    device.csr_transpose, then device.csr_elemwise(MX_OP_ADD) of the triangle and its transpose (the union
                     merge that an expansion without this family would need; f64 only)

usage: python tools/sym_timing.py [--warmup 5] [--iters 20] [--rows 1000000] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib  # noqa: E402
from matrixextra_amd import device as D  # noqa: E402


def upper_triangle(n, per_row):
    """per_row strictly-upper entries per row, sorted, spread over the row's tail; rows near the end keep fewer"""
    r = np.repeat(np.arange(n, dtype=np.int64), per_row)
    k = np.tile(np.arange(per_row, dtype=np.int64), n)
    stride = np.maximum((n - 1 - r) // per_row, 1)
    c = r + 1 + k * stride
    keep = c < n
    r, c = r[keep], c[keep]
    p = np.zeros(n + 1, dtype=np.int32)
    p[1:] = np.cumsum(np.bincount(r, minlength=n))
    x = ((np.arange(c.size) % 97) + 1).astype(np.float64)
    return p, c.astype(np.int32), x


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 4), round(float(np.min(times)), 4)


def copy_of(nbytes, warmup, iters):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), warmup, iters)


def time_kind(kind, p, j, x, n, warmup, iters):
    A = D.DeviceCSR.from_host(p, j, x if kind == "f64" else None, n)
    vb = 8 if kind == "f64" else 0
    out = []

    def report(what, med, best, written=None, **more):
        res = dict(kind=kind, what=what, n=n, nnz=A.nnz, median_ms=med, min_ms=best, **more)
        if written is not None:
            cmed, cbest = copy_of(written, warmup, iters)
            res.update(written_MB=round(written / 1e6, 1), copy_median_ms=cmed, copy_min_ms=cbest)
        print(json.dumps(res), flush=True)
        out.append(res)

    out_p, ws, nnz_out = D.csr_symmetric_count(A, "U")
    G = D.csr_symmetric_fill(A, "U", out_p, ws, nnz_out)
    # the expansion agrees with transpose + union merge before anything is timed (f64; the entries are disjoint)
    if kind == "f64":
        M = D.csr_elemwise(_lib.MX_OP_ADD, A, D.csr_transpose(A))
        assert M.nnz == G.nnz and torch.equal(M.indptr, G.indptr) and torch.equal(M.indices, G.indices)
        assert torch.equal(M.values, G.values)
    out_j, out_x = G.indices, G.values
    written = 4 * (n + 1) + (4 + vb) * nnz_out
    report("sym_count", *timed(lambda: D.csr_symmetric_count(A, "U"), warmup, iters), nnz_out=nnz_out)
    report("sym_fill", *timed(lambda: D.csr_symmetric_fill(A, "U", out_p, ws, nnz_out, out_j, out_x), warmup, iters),
           written=written, nnz_out=nnz_out, lanes=_lib.last_row_launch()[1])
    report("transpose_alone", *timed(lambda: D.csr_transpose(A), warmup, iters))
    if kind == "f64":
        report("transpose_merge", *timed(lambda: D.csr_elemwise(_lib.MX_OP_ADD, A, D.csr_transpose(A)), warmup, iters))
    U = D.csr_unit_triangular_to_general(A, "U")
    bufs = (U.indptr, U.indices, U.values)
    report("unit_tri", *timed(lambda: D.csr_unit_triangular_to_general(A, "U", bufs), warmup, iters),
           written=4 * (n + 1) + (4 + vb) * (A.nnz + n), nnz_out=A.nnz + n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    print("device:", _lib.device_name(), flush=True)
    p, j, x = upper_triangle(a.rows, 16)
    out = []
    for kind in ("f64", "pattern"):
        out += time_kind(kind, p, j, x, a.rows, a.warmup, a.iters)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
