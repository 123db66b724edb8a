#!/usr/bin/env python3
"""Device-event timing of mxd_coo_to_csr: 5 warm-up runs, then 20 timed runs, median and min.

Inputs at cfg2's shape: synth.csr_fixed(1_000_000, 100_000, 32) (32M f64 entries) expanded to COO and shuffled
with a seeded permutation, and the same triplets with 10 % of them duplicated (a copy of a random triplet with a
new value, shuffled in), so the merge pass runs.  Algorithmic bytes are 16 nnz read (i, j, x) + 4(m+1) + 12 nnz_out
written; the share is against the ~6.3 TB/s achievable HBM rate.

The timed region holds the call's host read-backs (flags, merged count), so it is an upper bound on the kernels'
time; take kernel time from a separate `rocprofv3 --kernel-trace --stats` run of this script.

usage: python tools/coo_timing.py [--warmup 5] [--iters 20] [--json out.json]
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

HBM_ACHIEVABLE = 6.3e12
SEED = 20260


def shuffled_coo(p, j, x, dup_share, seed=SEED):
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(p.size - 1, dtype=np.int32), np.diff(p))
    if dup_share:
        k = int(j.size * dup_share)
        src = rng.integers(0, j.size, k)
        i, j = np.concatenate([i, i[src]]), np.concatenate([j, j[src]])
        x = np.concatenate([x, rng.normal(size=k)])
    perm = rng.permutation(j.size)
    return i[perm], j[perm], x[perm]


def time_one(name, i, j, x, m, n, warmup, iters):
    lib = _lib.load()
    dev = "cuda"
    di, dj, dx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (i, j, x))
    nnz = int(i.size)
    ws = torch.empty(lib.mxd_coo_to_csr_workspace_bytes(nnz, n), dtype=torch.uint8, device=dev)
    op = torch.empty(m + 1, dtype=torch.int32, device=dev)
    oj = torch.empty(nnz, dtype=torch.int32, device=dev)
    ox = torch.empty(nnz, dtype=torch.float64, device=dev)
    out_nnz = C.c_int64(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.check(lib.mxd_coo_to_csr(m, n, C.c_void_p(di.data_ptr()), C.c_void_p(dj.data_ptr()),
                                      C.c_void_p(dx.data_ptr()), _lib.MX_F64, nnz, C.c_void_p(op.data_ptr()),
                                      C.c_void_p(oj.data_ptr()), C.c_void_p(ox.data_ptr()), C.c_void_p(ws.data_ptr()),
                                      C.byref(out_nnz), stream))

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
    nout = int(out_nnz.value)
    alg = 16 * nnz + 4 * (m + 1) + 12 * nout
    med, best = float(np.median(times)), float(np.min(times))
    res = dict(input=name, m=m, n=n, nnz=nnz, nnz_out=nout, median_ms=round(med, 4), min_ms=round(best, 4),
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
    out = [time_one("cfg2_shuffled", *shuffled_coo(p, j, x, 0.0), m, n, a.warmup, a.iters)]
    out.append(time_one("cfg2_shuffled+10pct_dup", *shuffled_coo(p, j, x, 0.1), m, n, a.warmup, a.iters))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
