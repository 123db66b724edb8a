#!/usr/bin/env python3
"""Device-event timing of the COO slice: device.coo_slice, i.e. the map build when a selector is
arbitrary, mxd_coo_slice_count (with its host read-back of the total) and mxd_coo_slice_fill.  5 warm-up runs, then
20 timed runs, median and min.

Input at cfg2's shape: synth.csr_fixed(1_000_000, 100_000, 32) (32M f64 entries) expanded to COO and shuffled with a
seeded permutation.  Selections:
  seq_x_seq        rows 100 001..900 000, columns 1..90 000 (affine x affine, no map)
  rows50_norep     a random 50 % of the rows, unsorted, no repeats; all columns
  rows50_rep       500 000 rows drawn with replacement (repeats), all columns
Algorithmic bytes: 8 B per triplet read by the count pass (i, j), 16 B per triplet read by the fill pass (i, j, x;
the offsets add 4 B), 16 B per output written (i, j, x); the share is against the ~6.3 TB/s achievable HBM rate.
The timed region holds the count's host read-back, so it is an upper bound on the kernels' time.

usage: python tools/coo_slice_timing.py [--warmup 5] [--iters 20] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib, device, synth  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
SEED = 20261


def time_one(name, di, dj, dx, m, n, rows, cols, warmup, iters):
    nnz = int(di.numel())

    def run():
        return device.coo_slice(di, dj, dx, m, n, rows, cols)

    for _ in range(warmup):
        out = run()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    nout = int(out[0].numel())
    alg = 8 * nnz + 16 * nnz + 16 * nout
    med, best = float(np.median(times)), float(np.min(times))
    res = dict(selection=name, m=m, n=n, nnz=nnz, nnz_out=nout, median_ms=round(med, 4), min_ms=round(best, 4),
               algorithmic_MB=round(alg / 1e6, 1), GBps_median=round(alg / med / 1e6, 1),
               hbm_share_median=round(alg / (med * 1e-3) / HBM_ACHIEVABLE, 3))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    print("device:", _lib.device_name(), flush=True)
    m, n = 1_000_000, 100_000
    p, j, x = synth.csr_fixed(m, n, 32)
    rng = np.random.default_rng(SEED)
    i = np.repeat(np.arange(m, dtype=np.int32), np.diff(p))
    perm = rng.permutation(j.size)
    di, dj, dx = (torch.from_numpy(np.ascontiguousarray(v[perm])).cuda() for v in (i, j, x))
    norep = torch.from_numpy((rng.permutation(m)[:m // 2] + 1).astype(np.int32)).cuda()
    rep = torch.from_numpy(rng.integers(1, m + 1, m // 2).astype(np.int32)).cuda()
    out = [time_one("seq_x_seq", di, dj, dx, m, n, ("seq", 100_000, 899_999), ("seq", 0, 89_999), a.warmup, a.iters),
           time_one("rows50_norep", di, dj, dx, m, n, ("map", norep), ("all",), a.warmup, a.iters),
           time_one("rows50_rep", di, dj, dx, m, n, ("map", rep), ("all",), a.warmup, a.iters)]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
