#!/usr/bin/env python3
"""Device-event timing of CSC * dense (device.csc_by_dense) on device-resident operands: 5 warm-up
runs, then 20 timed runs, median and min.

Input: a 100 000 x 4 000 dense operand (f64: 3.2 GB, int32: 1.6 GB, both far past the 256 MiB Infinity Cache) and a
CSC with 1 % of the cells stored (1 000 sorted rows per column, 4 M entries); NA cells are placed uniformly at random.
Cases: the NA-keeping path with 0 %, 0.1 % and 10 % NA cells, the values-only path, and the NA-keeping path with an
int32 dense operand at 0.1 % NA cells.

Algorithmic bytes (s = bytes per dense cell, F = m*n cells, T = output entries):
  count      s*F (the dense operand once) + F/8 (NA mask written) + 4 (n+1) + 4 nnz
  fill       F/8 (mask read) + 4 (n+1) + 12 nnz (indices, values) + s*nnz (one dense value per entry) + 12 T + 4 (n+1)
  unchanged  the fill is replaced by the values-only pass and two copies: 8 (n+1) + 8 nnz (p and indices copied)
             + 12 nnz + s*nnz + 8 nnz
  values-only path: 4 (n+1) + 12 nnz + s*nnz + 8 nnz (values) + 8 nnz (the copy of the indices)
The share is against the ~6.3 TB/s achievable HBM rate.  The NA-keeping timings hold the count's host read-back (one
synchronise), so they are upper bounds on the kernels' time.

usage: python tools/csc_dense_timing.py [--warmup 5] [--iters 20] [--json out.json]
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
    return float(np.median(times)), float(np.min(times))


def report(name, alg, med, best, **extra):
    res = dict(case=name, median_ms=round(med, 4), min_ms=round(best, 4), algorithmic_MB=round(alg / 1e6, 1),
               GBps_median=round(alg / med / 1e6, 1), hbm_share_median=round(alg / (med * 1e-3) / HBM_ACHIEVABLE, 3),
               **extra)
    print(json.dumps(res), flush=True)
    return res


def keep_bytes(s, m, n, nnz, total, changed):
    F = m * n
    count = s * F + F / 8 + 4 * (n + 1) + 4 * nnz
    if changed:
        return count + F / 8 + 4 * (n + 1) + 12 * nnz + s * nnz + 12 * total + 4 * (n + 1)
    return count + 8 * (n + 1) + 8 * nnz + 12 * nnz + s * nnz + 8 * nnz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.load()
    print("device:", _lib.device_name(), flush=True)
    m, n, per_col = 100_000, 4_000, 1_000
    p, i, x = synth.csr_fixed(n, m, per_col)              # the CSR of X^T = the CSC of X
    A = D.DeviceCSR.from_host(p, i, x, m)
    nnz = i.size
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    Dt = torch.randn(n, m, dtype=torch.float64, device="cuda", generator=gen)    # row-major D^T = column-major D
    Dm = Dt.t()
    out = []
    for frac in (0.0, 0.001, 0.1):
        if frac:
            Dt[torch.rand(n, m, device="cuda", generator=gen) < frac] = float("nan")
        na = int(torch.isnan(Dt).sum())
        rp, ri, rx = D.csc_by_dense(A, Dm, keep_na=True)
        total = ri.numel()
        med, best = timed(lambda: D.csc_by_dense(A, Dm, keep_na=True), a.warmup, a.iters)
        out.append(report(f"keep NAs, f64 dense, {frac * 100:g} % NA cells", keep_bytes(8, m, n, nnz, total, na > 0),
                          med, best, nnz=nnz, na_cells=na, out_entries=total))
        del rp, ri, rx
    med, best = timed(lambda: D.csc_by_dense(A, Dm, keep_na=False), a.warmup, a.iters)
    out.append(report("values only (ignore_na), f64 dense", 4 * (n + 1) + 12 * nnz + 8 * nnz + 8 * nnz + 8 * nnz,
                      med, best, nnz=nnz))
    del Dt, Dm
    torch.cuda.empty_cache()
    Di = torch.randint(-100, 100, (n, m), dtype=torch.int32, device="cuda", generator=gen)
    Di[torch.rand(n, m, device="cuda", generator=gen) < 0.001] = -2147483648
    na = int((Di == -2147483648).sum())
    rp, ri, rx = D.csc_by_dense(A, Di.t(), keep_na=True)
    total = ri.numel()
    med, best = timed(lambda: D.csc_by_dense(A, Di.t(), keep_na=True), a.warmup, a.iters)
    out.append(report("keep NAs, int32 dense, 0.1 % NA cells", keep_bytes(4, m, n, nnz, total, True), med, best,
                      nnz=nnz, na_cells=na, out_entries=total))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
