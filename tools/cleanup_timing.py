#!/usr/bin/env python3
"""Device-event timing of remove_sparse_zeros (mxd_compact_count + mxd_compact_fill) and of the index validation
(mxd_validate_indices) on device-resident operands: 5 warm-up runs, then 20 timed runs, median and
min.

Input: cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32 M f64 entries), with 0 %, 10 % and 90 % of the
values set to 0.  Algorithmic bytes of remove-zeros: values read twice (8 B each), indices and indptr read once,
12 B per kept entry and the new indptr written; with nothing removed only the count pass runs (values once).  The
validation reads the indices and the indptr once.  The share is against the ~6.3 TB/s achievable HBM rate.

The timed region holds each call's host read-back (the kept count, the flags), so it is an upper bound on the
kernels' time.

usage: python tools/cleanup_timing.py [--warmup 5] [--iters 20] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    print("device:", _lib.device_name(), flush=True)
    m, n = 1_000_000, 100_000
    p, j, x0 = synth.csr_fixed(m, n, 32)
    nnz = x0.size
    out = []
    for frac in (0.0, 0.1, 0.9):
        x = x0.copy()
        x[np.random.default_rng(3).random(nnz) < frac] = 0.0
        A = D.DeviceCSR.from_host(p, j, x, n)
        kept = int(np.count_nonzero(x))
        R = D.csr_remove_zeros(A)
        assert R.nnz == kept
        med, best = timed(lambda: D.csr_remove_zeros(A), a.warmup, a.iters)
        alg = 8 * nnz if kept == nnz else 8 * nnz * 2 + 4 * nnz + 4 * (m + 1) + 12 * kept + 4 * (m + 1)
        out.append(report(f"remove_zeros cfg2, {int(frac * 100)} % zeros", alg, med, best, nnz=nnz, kept=kept))
        del A, R
        torch.cuda.empty_cache()
    A = D.DeviceCSR.from_host(p, j, x0, n)
    ws = torch.empty(4, dtype=torch.int32, device=A.indptr.device)
    flags = C.c_int(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def validate():
        _lib.check(lib.mxd_validate_indices(C.c_void_p(A.indices.data_ptr()), nnz, n, C.c_void_p(A.indptr.data_ptr()),
                                            m + 1, m, C.c_void_p(ws.data_ptr()), C.byref(flags), stream))

    med, best = timed(validate, a.warmup, a.iters)
    assert flags.value == 0
    out.append(report("validate cfg2 (indices + indptr)", 4 * nnz + 4 * (m + 1), med, best, nnz=nnz))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
