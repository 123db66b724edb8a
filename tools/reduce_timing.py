#!/usr/bin/env python3
"""Device-event timing of the reductions: 5 warm-up runs, then 20 timed runs, median and min.

Inputs: cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32M f64 entries), and the same CSR with a dense first
column added (the cbind(1, X) shape: one column with m entries).  Timed, per input:

  row_sums            device.row_reduce(A, "sum")
  col_sums_fresh      device.col_reduce(A, "sum") with the column order built inside the timed region
  col_sums_cached     device.col_reduce(A, "sum") with the order cached on A (what a gradient step pays)
  norm_O              device.norm(A, "O") with the order cached (ends in the 8-byte read-back of the result)

Each stands next to `copy_ms`, a device-to-device copy of the bytes the call reads (`read_MB`: indptr or colptr, the
values, the permutation where there is one; for the fresh order also indptr and indices), and next to the route that
was available before this family existed, in the same process:

  parent_row_sums     device.spmv(A, ones)
  parent_col_sums     device.csr_transpose(A), then device.spmv(A^T, ones)

usage: python tools/reduce_timing.py [--warmup 5] [--iters 20] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib, synth  # noqa: E402
from matrixextra_amd import device as D  # noqa: E402


def with_dense_first_column(p, j, x):
    m = p.size - 1
    return (p + np.arange(m + 1, dtype=np.int32), np.insert(j + 1, p[:-1], 0).astype(np.int32),
            np.insert(x, p[:-1], 1.0))


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


def time_input(name, p, j, x, n, warmup, iters):
    A = D.DeviceCSR.from_host(p, j, x, n)
    m, nnz = A.m, A.nnz
    ones_n = torch.ones(n, dtype=torch.float64, device="cuda")
    ones_m = torch.ones(m, dtype=torch.float64, device="cuda")

    def fresh():
        A._order = None
        return D.col_reduce(A, "sum")

    def parent_cols():
        return D.spmv(D.csr_transpose(A), ones_m)

    reads = dict(row_sums=4 * (m + 1) + 8 * nnz,
                 col_sums_fresh=4 * (m + 1) + 4 * nnz + 4 * (n + 1) + 12 * nnz,
                 col_sums_cached=4 * (n + 1) + 12 * nnz,
                 norm_O=4 * (n + 1) + 12 * nnz + 8 * n)
    calls = dict(row_sums=lambda: D.row_reduce(A, "sum"), col_sums_fresh=fresh,
                 col_sums_cached=lambda: D.col_reduce(A, "sum"), norm_O=lambda: D.norm(A, "O"))
    # the routes agree before anything is timed
    want_cols = parent_cols().cpu().numpy()
    got_cols = D.col_reduce(A, "sum").cpu().numpy()
    assert np.allclose(got_cols, want_cols, rtol=1e-9, atol=1e-9 * float(np.abs(x).sum()) / n)
    assert np.allclose(D.row_reduce(A, "sum").cpu().numpy(), D.spmv(A, ones_n).cpu().numpy(), rtol=1e-9, atol=1e-9)
    out = []
    for what, fn in calls.items():
        med, best = timed(fn, warmup, iters)
        cmed, cbest = copy_of(reads[what], warmup, iters)
        res = dict(input=name, what=what, m=m, n=n, nnz=nnz, median_ms=med, min_ms=best,
                   read_MB=round(reads[what] / 1e6, 1), copy_median_ms=cmed, copy_min_ms=cbest,
                   GBps_median=round(reads[what] / med / 1e6, 1))
        print(json.dumps(res), flush=True)
        out.append(res)
    for what, fn in (("parent_row_sums", lambda: D.spmv(A, ones_n)), ("parent_col_sums", parent_cols)):
        med, best = timed(fn, warmup, iters)
        res = dict(input=name, what=what, m=m, n=n, nnz=nnz, median_ms=med, min_ms=best)
        print(json.dumps(res), flush=True)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the input (cfg2: 1,000,000)")
    a = ap.parse_args()
    print("device:", _lib.device_name(), flush=True)
    m, n = a.rows, 100_000
    p, j, x = synth.csr_fixed(m, n, 32)
    out = time_input("cfg2", p, j, x, n, a.warmup, a.iters)
    p2, j2, x2 = with_dense_first_column(p, j, x)
    out += time_input("cfg2+dense_col0", p2, j2, x2, n + 1, a.warmup, a.iters)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
