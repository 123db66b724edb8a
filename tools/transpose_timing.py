#!/usr/bin/env python3
"""Device-event timing of mxd_csr_transpose: 5 warm-up runs, then 20 timed runs, median and min.

Inputs: cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32M f64 entries), and the same CSR with a dense
first column added (the cbind(1, X) shape: one output row with m entries).  Algorithmic bytes are
4(m+1) + 12 nnz read + 4(n+1) + 12 nnz written; the share is against the ~6.3 TB/s achievable HBM rate.

The timed region holds the call's one host read-back (error / duplicate flags), so it is an upper bound on the
kernels' time; take kernel time from a separate `rocprofv3 --kernel-trace --stats` run of this script.

usage: python tools/transpose_timing.py [--warmup 5] [--iters 20] [--json out.json]
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

HBM_ACHIEVABLE = 6.3e12


def with_dense_first_column(p, j, x):
    m = p.size - 1
    return (p + np.arange(m + 1, dtype=np.int32), np.insert(j + 1, p[:-1], 0).astype(np.int32),
            np.insert(x, p[:-1], 1.0))


def time_one(name, p, j, x, n, warmup, iters):
    lib = _lib.load()
    A = D.DeviceCSR.from_host(p, j, x, n)
    m, nnz = A.m, A.nnz
    dev = A.indptr.device
    ws = torch.empty(lib.mxd_csr_transpose_workspace_bytes(nnz), dtype=torch.uint8, device=dev)
    op = torch.empty(n + 1, dtype=torch.int32, device=dev)
    oj = torch.empty(nnz, dtype=torch.int32, device=dev)
    ox = torch.empty(nnz, dtype=torch.float64, device=dev)
    out_nnz = C.c_int64(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.check(lib.mxd_csr_transpose(m, n, C.c_void_p(A.indptr.data_ptr()), C.c_void_p(A.indices.data_ptr()),
                                         C.c_void_p(A.values.data_ptr()), _lib.MX_F64, nnz, C.c_void_p(op.data_ptr()),
                                         C.c_void_p(oj.data_ptr()), C.c_void_p(ox.data_ptr()),
                                         C.c_void_p(ws.data_ptr()), C.byref(out_nnz), stream))

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
    assert out_nnz.value == nnz
    alg = 4 * (m + 1) + 12 * nnz + 4 * (n + 1) + 12 * nnz
    med, best = float(np.median(times)), float(np.min(times))
    res = dict(input=name, m=m, n=n, nnz=nnz, median_ms=round(med, 4), min_ms=round(best, 4),
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
    out = [time_one("cfg2", p, j, x, n, a.warmup, a.iters)]
    p2, j2, x2 = with_dense_first_column(p, j, x)
    out.append(time_one("cfg2+dense_col0", p2, j2, x2, n + 1, a.warmup, a.iters))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
