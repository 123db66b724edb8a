#!/usr/bin/env python3
"""Device-event timing of the NA-keeping RsparseMatrix (op) dense vector route (device.csr_by_dvec_keep_na, DESIGN.md
§4.12) on device-resident operands: 5 warm-up runs, then 20 timed runs, median, min and max.

Input: cfg2's matrix (1 M x 100 k, 32 entries per row, 32 M entries) and `X / v`.  Cases:
  rows 0         row-ruled regime, length(v) = nrow, no zero in v: every row plain
  rows 0.01 %    the same with 0.01 % of v zero: those rows come out with all 100 k columns
  flat 0         flat regime, length(v) = nrow + 1, nothing special: the input structure and the values-only product
  flat 0.01 %    the same with 0.01 % of the positions zero: their cells outside X's pattern are added
  yardstick      the least the route must move when nothing is special: the values-only mxd_csr_by_dvec on the same X
                 and a device copy of `indices`.  Its own spread, max / min over its runs, is the margin for the
                 ratios of medians `rows 0 / yardstick` and `flat 0 / yardstick`.
The cases with special values have no yardstick.  The timings hold the routes' host read-backs (one synchronise in the
row-ruled regime, up to three in the flat one), so they are upper bounds on the kernels' time.

usage: python tools/dvec_na_timing.py [--warmup 5] [--iters 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib, synth  # noqa: E402
from matrixextra_amd import device as D  # noqa: E402


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


def report(name, t, **extra):
    res = dict(case=name, median_ms=round(t[0], 4), min_ms=round(t[1], 4), max_ms=round(t[2], 4), **extra)
    print(json.dumps(res), flush=True)
    return res


def yardstick(A, v):
    out = torch.empty(max(A.nnz, 1), dtype=torch.float64, device=v.device)
    _lib.check(_lib.load().mxd_csr_by_dvec(A.m, A.K, A.nnz, D._dp(A.indptr), D._dp(A.indices), D._dp(A.values),
                                           D._dp(v), v.numel(), _lib.MX_DV_OPS["/"], 1, D._dp(out), D._stream()))
    return out, A.indices.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    _lib.load()
    print("device:", _lib.device_name(), flush=True)
    m, K, per_row = a.rows, 100_000, 32
    p, j, x = synth.csr_fixed(m, K, per_row)
    A = D.DeviceCSR.from_host(p, j, x, K)
    rng = np.random.default_rng(12)
    out = []

    def vector(L, share):
        v = rng.uniform(0.5, 2.0, size=L)
        if share:
            v[rng.choice(L, max(int(L * share), 1), replace=False)] = 0.0
        return torch.from_numpy(v).cuda()

    ratios = {}
    for name, L in (("rows", m), ("flat", m + 1)):
        v0 = vector(L, 0.0)
        t_y = timed(lambda: yardstick(A, v0), a.warmup, a.iters)
        out.append(report(f"yardstick for {name}: values-only mxd_csr_by_dvec + copy of indices", t_y, length=L))
        rp, rj, rx = D.csr_by_dvec_keep_na(A, v0, "/")
        assert rj.numel() == A.nnz
        t0 = timed(lambda: D.csr_by_dvec_keep_na(A, v0, "/"), a.warmup, a.iters)
        out.append(report(f"{name} 0: nothing special", t0, length=L, out_entries=int(rj.numel())))
        ratios[name] = dict(case=f"{name} 0 / yardstick", ratio_of_medians=round(t0[0] / t_y[0], 3),
                            yardstick_spread_max_over_min=round(t_y[2] / t_y[1], 3),
                            within_margin=bool(t0[0] / t_y[0] <= t_y[2] / t_y[1]))
        print(json.dumps(ratios[name]), flush=True)
        out.append(ratios[name])
        del rp, rj, rx
        v1 = vector(L, 1e-4)
        rp, rj, rx = D.csr_by_dvec_keep_na(A, v1, "/")
        T = int(rj.numel())
        del rp, rj, rx
        t1 = timed(lambda: D.csr_by_dvec_keep_na(A, v1, "/"), a.warmup, a.iters)
        out.append(report(f"{name} 0.01 %: zeros in v; no yardstick, unmeasured against anything", t1, length=L,
                          special=int((v1 == 0).sum().item()), out_entries=T))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
