#!/usr/bin/env python3
"""Device-event timing of the transposed products: 5 warm-up runs, then 20 timed runs, median and min.

Inputs: cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32M f64 entries), and the same CSR with a dense first
column added (the cbind(1, X) shape: one column with m entries).  Timed, per input:

  X^T v
    spmv_t_cached        device.spmv_t(A, v) with the column order and the entry rows cached on A (a gradient step)
    spmv_t_fresh         the same with the order and the rows built inside the timed region
    product_col_reduce   X * v into a values buffer (mxd_csr_by_dvec), then device.col_reduce with the cached order:
                         the route that writes and re-reads the product
    transpose_spmv       device.csr_transpose(A), then device.spmv(A^T, v): the route without a cached order
    copy_ms              a device-to-device copy of the bytes spmv_t_cached reads (`read_MB`: colptr, the permutation,
                         the entry rows, the values and v)
  X^T B, B 1_000_000 x 128 f64
    transposed_cached    A.transposed() from the cached order and rows: one gather of the values
    spmm_on_transposed   device.spmm on it
    csr_transpose        device.csr_transpose(A): the radix sort
    spmm_on_csr_transpose  device.spmm on that

usage: python tools/tprod_timing.py [--warmup 5] [--iters 20] [--json out.json]
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


def time_input(name, p, j, x, n, ncols_B, warmup, iters):
    A = D.DeviceCSR.from_host(p, j, x, n)
    m, nnz = A.m, A.nnz
    v = torch.from_numpy(synth.dense_normal(m, 1).reshape(-1)).cuda()
    product = torch.empty(nnz, dtype=torch.float64, device="cuda")
    Y = D.DeviceCSR(A.indptr, A.indices, product, m, n, nnz)
    mult = _lib.MX_DV_OPS["*"]

    def fresh():
        A._order = A._rows = None
        return D.spmv_t(A, v)

    def product_then_reduce():
        D._call("mxd_csr_by_dvec", m, n, nnz, D._dp(A.indptr), D._dp(A.indices), D._dp(A.values), D._dp(v), m, mult, 1,
                D._dp(product))
        return D.col_reduce(Y, "sum", order=A.column_order())

    def transpose_spmv():
        return D.spmv(D.csr_transpose(A), v)

    # the routes agree before anything is timed: the fused product is the reduction of the written-out one, bit for bit
    got = D.spmv_t(A, v)
    assert torch.equal(got.view(torch.int64), product_then_reduce().view(torch.int64))
    scale = 1e-9 * float(np.abs(x).sum()) / n
    assert np.allclose(got.cpu().numpy(), transpose_spmv().cpu().numpy(), rtol=1e-9, atol=scale)

    out = []

    def report(what, fn, read=None):
        med, best = timed(fn, warmup, iters)
        res = dict(input=name, what=what, m=m, n=n, nnz=nnz, median_ms=med, min_ms=best)
        if read is not None:
            cmed, cbest = copy_of(read, warmup, iters)
            res.update(read_MB=round(read / 1e6, 1), copy_median_ms=cmed, copy_min_ms=cbest,
                       GBps_median=round(read / med / 1e6, 1))
        print(json.dumps(res), flush=True)
        out.append(res)

    report("spmv_t_cached", lambda: D.spmv_t(A, v), read=4 * (n + 1) + 16 * nnz + 8 * m)
    report("spmv_t_fresh", fresh)
    report("product_col_reduce", product_then_reduce)
    report("transpose_spmv", transpose_spmv)

    B = torch.from_numpy(synth.dense_normal(m, ncols_B)).cuda()
    T = A.transposed()
    S = D.csr_transpose(A)
    C1, C2 = D.spmm(T, B), D.spmm(S, B)
    assert torch.equal(C1.view(torch.int64), C2.view(torch.int64))         # the same kernel on identical arrays
    del C1, C2
    Cout = torch.empty((n, ncols_B), dtype=torch.float64, device="cuda")
    report("transposed_cached", lambda: A.transposed())
    report("spmm_on_transposed", lambda: D.spmm(T, B, out=Cout))
    report("csr_transpose", lambda: D.csr_transpose(A))
    report("spmm_on_csr_transpose", lambda: D.spmm(S, B, out=Cout))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the input (cfg2: 1,000,000)")
    ap.add_argument("--n", type=int, default=128, help="columns of B in X^T B")
    a = ap.parse_args()
    print("device:", _lib.device_name(), flush=True)
    m, n = a.rows, 100_000
    p, j, x = synth.csr_fixed(m, n, 32)
    out = time_input("cfg2", p, j, x, n, a.n, a.warmup, a.iters)
    p2, j2, x2 = with_dense_first_column(p, j, x)
    out += time_input("cfg2+dense_col0", p2, j2, x2, n + 1, a.n, a.warmup, a.iters)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
