#!/usr/bin/env python3
"""Device-event timing of matrix * sparseVector (mxd_dense_by_svec_count / _fill / _dense) on
device-resident operands: 5 warm-up runs, then 20 timed runs, median, min and max.

Input: a 1 000 000 x 128 f64 X (1.02 GB, column-major, far past the 256 MiB Infinity Cache) and a vector of length
nrows that stores every other position (500 000 rows, 64 M output entries, 768 MB of indices and values).
Cases: the CSR route keeping NAs (0.1 % of X's cells NaN) and ignoring them, and the dense route A (length = cells, a
tenth of the positions stored, NAs kept).

Yardstick, timed in the same run next to each case: a hipMemsetAsync of the case's output bytes plus a device-to-device
copy of X's bytes, i.e. what the runtime needs to write that much and to read and write X once.  No threshold is set:
the ratio case / yardstick is reported with the yardstick's own max / min over its runs as the margin.  The CSR
timings hold the count's host read-back (one synchronise).

usage: python tools/dense_svec_timing.py [--warmup 5] [--iters 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib  # noqa: E402
from matrixextra_amd._lib import check  # noqa: E402
from matrixextra_amd.device import _dp, _stream  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    print("device:", _lib.device_name(), flush=True)
    nrows, ncols = 1_000_000, 128
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    Xc = torch.randn(ncols, nrows, dtype=torch.float64, device="cuda", generator=gen)     # row-major X^T = column-major X
    Xc[torch.rand(ncols, nrows, device="cuda", generator=gen) < 0.001] = float("nan")
    Xcopy = torch.empty_like(Xc)
    x_bytes = Xc.numel() * 8
    out = []

    def yardstick(*outputs):
        def run():
            for buf, nbytes in outputs:
                check(lib.mx_dev_memset(_dp(buf), 0, nbytes, _stream()))
            Xcopy.copy_(Xc)
        return run

    def report(name, case, yard, out_bytes, **extra):
        res = dict(case=name, median_ms=round(case[0], 4), min_ms=round(case[1], 4), max_ms=round(case[2], 4),
                   yardstick_median_ms=round(yard[0], 4), yardstick_min_ms=round(yard[1], 4),
                   yardstick_max_ms=round(yard[2], 4), ratio_of_medians=round(case[0] / yard[0], 3),
                   yardstick_max_over_min=round(yard[2] / yard[1], 3), x_MB=round(x_bytes / 1e6, 1),
                   out_MB=round(out_bytes / 1e6, 1), **extra)
        print(json.dumps(res), flush=True)
        out.append(res)

    # ---- the CSR route (B): length = nrows, every other position stored
    vi = torch.arange(1, nrows + 1, 2, dtype=torch.int32, device="cuda")
    vx = torch.randn(vi.numel(), dtype=torch.float64, device="cuda", generator=gen)
    ws = torch.empty(lib.mxd_dense_by_svec_workspace_bytes(nrows, nrows), dtype=torch.uint8, device="cuda")
    out_p = torch.empty(nrows + 1, dtype=torch.int32, device="cuda")
    cap = vi.numel() * ncols + Xc.numel() // 500                     # full rows and room for the NaN cells of the others
    out_j = torch.empty(cap, dtype=torch.int32, device="cuda")
    out_x = torch.empty(cap, dtype=torch.float64, device="cuda")
    for keep in (1, 0):
        total = C.c_int64(0)

        def run():
            check(lib.mxd_dense_by_svec_count(nrows, ncols, _dp(Xc), 0, _dp(vi), vi.numel(), nrows, keep, _dp(ws),
                                              _dp(out_p), C.byref(total), _stream()))
            assert total.value <= cap
            check(lib.mxd_dense_by_svec_fill(nrows, ncols, _dp(Xc), 0, _dp(vx), nrows, keep, _dp(ws), _dp(out_p),
                                             _dp(out_j), _dp(out_x), _stream()))
        case = timed(run, a.warmup, a.iters)
        out_bytes = 12 * total.value + 4 * (nrows + 1)
        yard = timed(yardstick((out_x, 8 * total.value), (out_j, 4 * total.value), (out_p, 4 * (nrows + 1))),
                     a.warmup, a.iters)
        report(f"CSR route, length = nrows, half the positions stored, {'NAs kept' if keep else 'NAs ignored'}", case,
               yard, out_bytes, out_entries=total.value)
    del out_j, out_x, ws

    # ---- the dense route (A): length = cells, a tenth of the positions stored, NAs kept
    F = nrows * ncols
    vi = torch.arange(1, F + 1, 10, dtype=torch.int32, device="cuda")
    vx = torch.randn(vi.numel(), dtype=torch.float64, device="cuda", generator=gen)
    ws = torch.empty(lib.mxd_dense_by_svec_workspace_bytes(0, F), dtype=torch.uint8, device="cuda")
    dense = torch.empty(F, dtype=torch.float64, device="cuda")

    def run_a():
        check(lib.mxd_dense_by_svec_dense(nrows, ncols, _dp(Xc), 0, _dp(vi), vi.numel(), _dp(vx), F, 1, _dp(ws),
                                          _dp(dense), _stream()))
    case = timed(run_a, a.warmup, a.iters)
    yard = timed(yardstick((dense, F * 8)), a.warmup, a.iters)
    report("dense route A, length = cells, a tenth of the positions stored, NAs kept", case, yard, F * 8,
           stored=vi.numel())
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
