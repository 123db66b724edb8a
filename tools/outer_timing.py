#!/usr/bin/env python3
"""Device-event timing of the outer products of `%*%` and the float32 row-vector product (device.csr_outer_dense,
csr_outer_svec, rowvec_by_csc) on device-resident operands: 5 warm-up runs, then 20 timed runs,
median, min and max.

Cases:
  dense outer   a one-column matrix of cfg2's 1 M rows, half of them stored, against a dense f64 vector of length 128
  sparse outer  the same matrix against a sparse vector of length 128 that stores half of its positions
  row vector    a float32 vector of 100 k against cfg2's CSR (1 M x 100 k, 32 entries per row) read as the (p, i, x) of
                a CSC with 1 M columns
Each case is followed by its yardstick from the same run: a hipMemsetAsync of the bytes the case writes (12 B per
output entry for the outer products, 4 B per column for the row vector), the time a pure write of that output takes
on the same card.  The row vector reads far more than it writes (12 B per entry), so its algorithmic bytes are shown
too.  The outer products' timings hold the count's host read-backs (one synchronise for the dense one, two for the
sparse one) and the allocation of the output tensors, so they are upper bounds on the kernels' time.

usage: python tools/outer_timing.py [--warmup 5] [--iters 20] [--json out.json]
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

HBM_ACHIEVABLE = 6.3e12


def timed(run, warmup, iters):
    for _ in range(warmup):
        run()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def report(name, written, t, **extra):
    med, best, worst = t
    res = dict(case=name, median_ms=round(med, 4), min_ms=round(best, 4), max_ms=round(worst, 4),
               written_MB=round(written / 1e6, 1), write_GBps_median=round(written / med / 1e6, 1),
               hbm_share_median=round(written / (med * 1e-3) / HBM_ACHIEVABLE, 3), **extra)
    print(json.dumps(res), flush=True)
    return res


def pure_write(nbytes, warmup, iters):
    lib = _lib.load()
    buf = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    t = timed(lambda: _lib.check(lib.mx_dev_memset(D._dp(buf), 0, nbytes, D._stream())), warmup, iters)
    del buf
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    _lib.load()
    print("device:", _lib.device_name(), flush=True)
    m, dim = a.rows, 128
    rng = np.random.default_rng(11)
    full = rng.random(m) < 0.5
    p = np.concatenate([[0], np.cumsum(full)]).astype(np.int32)
    stored = int(p[-1])
    X = D.DeviceCSR.from_host(p, np.zeros(stored, np.int32), rng.uniform(0.5, 2.0, size=stored), 1)
    out = []

    v = torch.from_numpy(rng.normal(size=dim)).cuda()
    rp, rj, rx = D.csr_outer_dense(X, v)
    T = int(rj.numel())
    assert T == stored * dim and int(rp[-1]) == T
    del rp, rj, rx
    t = timed(lambda: D.csr_outer_dense(X, v), a.warmup, a.iters)
    out.append(report("dense outer: 1 M rows, half stored, f64 vector of 128", 12 * T, t, rows=m, stored=stored,
                      out_entries=T))
    out.append(report("yardstick: memset of the dense outer product's output", 12 * T, pure_write(12 * T, a.warmup, a.iters)))

    vi = torch.from_numpy((np.flatnonzero(rng.random(dim) < 0.5) + 1).astype(np.int32)).cuda()
    vx = torch.from_numpy(rng.normal(size=int(vi.numel()))).cuda()
    rp, ri, rx = D.csr_outer_svec(X, vi, vx, dim)
    T = int(ri.numel())
    assert T == stored * int(vi.numel())
    del rp, ri, rx
    t = timed(lambda: D.csr_outer_svec(X, vi, vx, dim), a.warmup, a.iters)
    out.append(report("sparse outer: the same matrix, dsparseVector of length 128, half stored", 12 * T, t, rows=m,
                      stored=stored, stored_positions=int(vi.numel()), out_entries=T))
    out.append(report("yardstick: memset of the sparse outer product's output", 12 * T, pure_write(12 * T, a.warmup, a.iters)))
    del X

    K, per_row = 100_000, 32
    cp, ci, cx = synth.csr_fixed(m, K, per_row)
    Y = D.DeviceCSR.from_host(cp, ci, cx, K)
    rv = torch.from_numpy(rng.normal(size=K).astype(np.float32)).cuda()
    t = timed(lambda: D.rowvec_by_csc(rv, Y), a.warmup, a.iters)
    alg = 4 * (m + 1) + 12 * ci.size + 4 * K + 4 * m
    out.append(report("row vector: float32[100 k] x cfg2's arrays as a CSC of 1 M columns", 4 * m, t, nnz=int(ci.size),
                      algorithmic_MB=round(alg / 1e6, 1), algorithmic_GBps_median=round(alg / t[0] / 1e6, 1),
                      algorithmic_hbm_share_median=round(alg / (t[0] * 1e-3) / HBM_ACHIEVABLE, 3)))
    out.append(report("yardstick: memset of the row vector product's output", 4 * m, pure_write(4 * m, a.warmup, a.iters)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
