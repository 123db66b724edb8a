#!/usr/bin/env python3
"""Device-event timing of mxd_coo_sort against mxd_coo_to_csr on the same input in the same run:
5 warm-up runs, then 20 timed runs, median and min.

Input at cfg2's shape: synth.csr_fixed(1_000_000, 100_000, 32) (32M entries) expanded to COO and shuffled with the
seeded permutation of tools/coo_timing.py.  Cases: the sort with f64 values, the sort of the pattern alone, the sort of
the already-sorted triplets (the reduction only), and the yardstick coo_to_csr with f64 values.  The sort works in
place, so every run starts from a fresh device copy of the shuffled triplets made outside the timed region.
Algorithmic bytes of the sort: the triplets read once and written once.

The timed region holds the call's host read-back (the reduction's words), so it is an upper bound on the kernels' time.

usage: python tools/coo_sort_timing.py [--warmup 5] [--iters 20] [--json profiles/coo_sort_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from coo_timing import HBM_ACHIEVABLE, shuffled_coo  # noqa: E402
from matrixextra_amd import _lib, device as D, synth  # noqa: E402


def timed(run, reset, warmup, iters):
    for _ in range(warmup):
        reset()
        run()
    times = []
    for _ in range(iters):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def report(name, nnz, alg, med, best, **extra):
    res = dict(case=name, nnz=nnz, median_ms=round(med, 4), min_ms=round(best, 4), algorithmic_MB=round(alg / 1e6, 1),
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
    print("device:", _lib.device_name(), flush=True)
    lib = _lib.load()
    m, n = 1_000_000, 100_000
    p, j, x = synth.csr_fixed(m, n, 32)
    i, j, x = shuffled_coo(p, j, x, 0.0)
    nnz = int(i.size)
    src = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (i, j, x)]
    work = [torch.empty_like(t) for t in src]

    def reset():
        for w, s in zip(work, src):
            w.copy_(s)

    out = []
    state = {}
    for name, with_values in (("sort_f64", True), ("sort_pattern", False)):
        def run():
            state["sorted"] = D.coo_sort(work[0], work[1], work[2] if with_values else None)
        med, best = timed(run, reset, a.warmup, a.iters)
        assert state["sorted"] is False
        out.append(report(name, nnz, (32 if with_values else 16) * nnz, med, best))
    # the sorted triplets (left in `work` by the last f64 run): the reduction alone
    reset()
    D.coo_sort(*work)
    done = [t.clone() for t in work]
    med, best = timed(lambda: state.update(sorted=D.coo_sort(*done)), lambda: None, a.warmup, a.iters)
    assert state["sorted"] is True
    out.append(report("sort_f64_already_sorted", nnz, 8 * nnz, med, best))

    # the yardstick: coo_to_csr of the same shuffled triplets
    ws = torch.empty(lib.mxd_coo_to_csr_workspace_bytes(nnz, n), dtype=torch.uint8, device="cuda")
    op = torch.empty(m + 1, dtype=torch.int32, device="cuda")
    oj = torch.empty(nnz, dtype=torch.int32, device="cuda")
    ox = torch.empty(nnz, dtype=torch.float64, device="cuda")
    out_nnz = C.c_int64(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def to_csr():
        _lib.check(lib.mxd_coo_to_csr(m, n, C.c_void_p(src[0].data_ptr()), C.c_void_p(src[1].data_ptr()),
                                      C.c_void_p(src[2].data_ptr()), _lib.MX_F64, nnz, C.c_void_p(op.data_ptr()),
                                      C.c_void_p(oj.data_ptr()), C.c_void_p(ox.data_ptr()), C.c_void_p(ws.data_ptr()),
                                      C.byref(out_nnz), stream))
    med, best = timed(to_csr, lambda: None, a.warmup, a.iters)
    out.append(report("coo_to_csr_f64", nnz, 16 * nnz + 4 * (m + 1) + 12 * int(out_nnz.value), med, best,
                      nnz_out=int(out_nnz.value)))
    # the sort and the conversion agree on the order
    assert torch.equal(done[1], oj) and torch.equal(done[2].view(torch.int64), ox.view(torch.int64))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
