#!/usr/bin/env python3
"""Device-event timing of the CSR assignment kernels (mxd_csr_assign_count + _fill, mxd_csr_replace_rows_count + _fill;
DESIGN.md §4.16) on device-resident operands: 5 warm-up runs, then 20 timed runs, median and min.

Input: cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32 M f64 entries).  Four calls:
  X[1 % of the rows (arbitrary), 1 000 arbitrary columns] <- 0
  X[, 16 arbitrary columns] <- 1
  X[a row sequence of 10 %, ] <- 0
  X[10 % of the rows (arbitrary), ] <- Y, Y's rows of the same mean length
Each call is timed next to a device-to-device copy of as many bytes as its output CSR holds (indptr, indices, values):
an operation that rewrites the matrix cannot be faster than that copy, so the ratio says how far from the floor it is.
The timed region holds the count pass's host read-back.  No threshold is set: the tool reports.

usage: python tools/assign_timing.py [--warmup 5] [--iters 20] [--json out.json]
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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Axis:
    """mx_coo_axis of a 0-based selector: None = all of n, (lo, hi) a range, an array an arbitrary set."""

    def __init__(self, sel, n):
        self.sorted = None
        if sel is None or isinstance(sel, tuple):
            lo, hi = (0, n - 1) if sel is None else sel
            self.n, self.c = hi - lo + 1, _lib.CooAxis(_lib.MX_AXIS_AFFINE, lo, hi, 0, 0, None, None)
            return
        keys = np.asarray(sel, dtype=np.int64) + 1
        nmap = int(keys.max()) + 1
        start = np.zeros(nmap + 1, dtype=np.int32)
        start[1:] = np.cumsum(np.bincount(keys, minlength=nmap))
        self.start, self.pos = dev(start), dev(np.argsort(keys, kind="stable").astype(np.int32))
        self.sorted = dev(np.sort(keys - 1).astype(np.int32))
        self.n = keys.size
        self.c = _lib.CooAxis(_lib.MX_AXIS_MAP, 0, 0, 0, nmap, self.start.data_ptr(), self.pos.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    print("device:", _lib.device_name(), flush=True)
    m, n, per_row = 1_000_000, 100_000, 32
    p, j, x = synth.csr_fixed(m, n, per_row)
    nnz = int(j.size)
    assert np.all(np.diff(j[:per_row * 1000].reshape(1000, per_row), axis=1) > 0), "cfg2's rows are sorted"
    dp, dj, dx = dev(p), dev(j), dev(x)
    rng = np.random.default_rng(5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.mxd_gather_workspace_bytes(m), dtype=torch.uint8, device="cuda")
    new_p = torch.empty(m + 1, dtype=torch.int32, device="cuda")
    cap = nnz + 16 * m
    new_j = torch.empty(cap, dtype=torch.int32, device="cuda")
    new_x = torch.empty(cap, dtype=torch.float64, device="cuda")
    avg = nnz / m
    out = []

    def floor_copy(total):
        nbytes = 4 * (m + 1) + 12 * total
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        med, best = timed(lambda: dst.copy_(src), a.warmup, a.iters)
        return nbytes, med, best

    def report(name, total, hits, med, best):
        nbytes, cmed, cbest = floor_copy(total)
        res = dict(case=name, median_ms=round(med, 4), min_ms=round(best, 4), out_entries=total, hits=hits,
                   out_MB=round(nbytes / 1e6, 1), copy_median_ms=round(cmed, 4), copy_min_ms=round(cbest, 4),
                   times_the_copy=round(med / cmed, 2))
        print(json.dumps(res), flush=True)
        out.append(res)

    def scalar_case(name, rows, cols, value):
        ai, aj = Axis(rows, m), Axis(cols, n)
        is_const = int(value != 0)
        total, hits = C.c_int64(0), C.c_int64(0)

        def run():
            _lib.check(lib.mxd_csr_assign_count(m, n, vp(dp), vp(dj), nnz, C.byref(ai.c), C.byref(aj.c), ai.n, aj.n,
                                                is_const, avg, vp(new_p), vp(ws), C.byref(total), C.byref(hits),
                                                stream))
            assert total.value <= cap
            _lib.check(lib.mxd_csr_assign_fill(m, n, vp(dp), vp(dj), vp(dx), C.byref(ai.c), C.byref(aj.c),
                                               vp(aj.sorted), aj.n, is_const, value, avg, vp(new_p), vp(new_j),
                                               vp(new_x), stream))
        med, best = timed(run, a.warmup, a.iters)
        report(name, int(total.value), int(hits.value), med, best)

    scalar_case("X[1 % of rows, 1000 arbitrary cols] <- 0", rng.choice(m, size=m // 100, replace=False),
                rng.choice(n, size=1000, replace=False), 0.0)
    scalar_case("X[, 16 arbitrary cols] <- 1", None, rng.choice(n, size=16, replace=False), 1.0)
    scalar_case("X[rowseq of 10 %, ] <- 0", (m // 2, m // 2 + m // 10 - 1), None, 0.0)

    k = m // 10
    vpn, vjn, vxn = synth.csr_fixed(k, n, per_row)
    dvp, dvj, dvx = dev(vpn), dev(vjn), dev(vxn)
    ai = Axis(rng.choice(m, size=k, replace=False), m)
    total = C.c_int64(0)

    def replace():
        _lib.check(lib.mxd_csr_replace_rows_count(m, vp(dp), C.byref(ai.c), k, vp(dvp), vp(new_p), vp(ws),
                                                  C.byref(total), stream))
        assert total.value <= cap
        _lib.check(lib.mxd_csr_replace_rows_fill(m, vp(dp), vp(dj), vp(dx), C.byref(ai.c), k, vp(dvp), vp(dvj), vp(dvx),
                                                 avg, vp(new_p), vp(new_j), vp(new_x), stream))
    med, best = timed(replace, a.warmup, a.iters)
    report("X[10 % of rows, ] <- Y (rows of equal mean length)", int(total.value), 0, med, best)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
