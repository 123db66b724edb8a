#!/usr/bin/env python3
"""Device-event timing of NA injection on device-resident operands: 5 warm-up runs, then 20 timed
runs, median and min.

Input: cfg2's matrix, synth.csr_fixed(1_000_000, 100_000, 32) (32 M f64 entries).  Selectors: 1 000 NA rows (random,
ascending), 16 NA columns, and both.  Two routes:
  COO   the matrix as shuffled triplets through device.coo_inject_na (mxd_coo_inject_na_count + _fill)
  CSR   the matrix as it is through the two scalar assignments of NA_real_ that inject_NAs makes of the lists
        (mxd_csr_assign_count + _fill over the NA rows and all columns, then over all rows and the NA columns)
Each case is timed next to a device-to-device copy of as many bytes as its output holds (COO: 16 B per entry; CSR:
indptr and 12 B per entry): an operation that writes its output cannot be faster than that copy, so the ratio says
how far from the floor it is.  The COO case also reports its passes on their own: the maps and the kept count with its
read-back, the kept fill, and the NA block.  The timed regions hold the count passes' host read-backs.  No threshold
is set: the tool reports.

usage: python tools/na_slice_timing.py [--warmup 5] [--iters 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib, device, synth  # noqa: E402

SEED = 20418
NA_REAL = np.frombuffer(np.uint64(0x7FF00000000007A2).tobytes(), dtype=np.float64)[0]


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


def copy_of(nbytes, warmup, iters):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), warmup, iters)


def axis_of(sel, n):
    """(mx_coo_axis, its length, tensors to keep alive, ascending device list) of a 0-based ascending selector"""
    if sel is None:
        return _lib.CooAxis(_lib.MX_AXIS_AFFINE, 0, n - 1, 0, 0, None, None), n, (), None
    keys = np.asarray(sel, dtype=np.int64) + 1
    nmap = int(keys.max()) + 1
    start = np.zeros(nmap + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(keys, minlength=nmap))
    dstart, dpos, dsorted = dev(start), dev(np.arange(keys.size, dtype=np.int32)), dev(np.asarray(sel, dtype=np.int32))
    ax = _lib.CooAxis(_lib.MX_AXIS_MAP, 0, 0, 0, nmap, dstart.data_ptr(), dpos.data_ptr())
    return ax, int(keys.size), (dstart, dpos), dsorted


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
    rng = np.random.default_rng(SEED)
    rows_na = np.sort(rng.choice(m, size=1000, replace=False)).astype(np.int32)
    cols_na = np.sort(rng.choice(n, size=16, replace=False)).astype(np.int32)
    none = np.zeros(0, dtype=np.int32)
    cases = [("1000 NA rows", rows_na, none), ("16 NA columns", none, cols_na), ("1000 NA rows, 16 NA columns", rows_na, cols_na)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []

    def report(res):
        print(json.dumps(res), flush=True)
        out.append(res)

    # ---- COO
    i = np.repeat(np.arange(m, dtype=np.int32), np.diff(p))
    perm = rng.permutation(nnz)
    di, dj, dx = (dev(v[perm]) for v in (i, j, x))
    for name, rna, cna in cases:
        drna, dcna = dev(rna), dev(cna)
        total = int(device.coo_inject_na(di, dj, dx, m, n, drna, dcna)[0].numel())
        med, best = timed(lambda: device.coo_inject_na(di, dj, dx, m, n, drna, dcna), a.warmup, a.iters)
        cmed, cbest = copy_of(16 * total, a.warmup, a.iters)
        # the passes on their own, on buffers allocated once
        ws = torch.empty(lib.mxd_compact_workspace_bytes(nnz), dtype=torch.uint8, device="cuda")
        maps = torch.empty(4 + m + n + max(m, n), dtype=torch.int32, device="cuda")
        oi = torch.empty(total, dtype=torch.int32, device="cuda")
        oj, ox = torch.empty_like(oi), torch.empty(total, dtype=torch.float64, device="cuda")
        got = C.c_int64(0)

        def count():
            _lib.check(lib.mxd_coo_inject_na_count(m, n, vp(di), vp(dj), nnz, vp(drna), rna.size, vp(dcna), cna.size,
                                                   vp(ws), vp(maps), C.byref(got), stream))

        def fill():
            _lib.check(lib.mxd_coo_inject_na_fill(m, n, vp(di), vp(dj), vp(dx), _lib.MX_F64, nnz, vp(drna), rna.size,
                                                  vp(dcna), cna.size, vp(ws), vp(maps), vp(oi), vp(oj), vp(ox),
                                                  stream))
        count_med, _ = timed(count, a.warmup, a.iters)
        assert got.value == total
        fill_med, _ = timed(fill, a.warmup, a.iters)
        kept = total - (rna.size * n + cna.size * (m - rna.size))
        report(dict(route="COO", case=name, median_ms=round(med, 4), min_ms=round(best, 4), out_entries=total,
                    kept_entries=kept, out_MB=round(16 * total / 1e6, 1), copy_median_ms=round(cmed, 4),
                    copy_min_ms=round(cbest, 4), times_the_copy=round(med / cmed, 2),
                    count_pass_median_ms=round(count_med, 4), fill_pass_median_ms=round(fill_med, 4),
                    allocation_and_rest_ms=round(med - count_med - fill_med, 4)))
        del ws, maps, oi, oj, ox, drna, dcna
    del di, dj, dx

    # ---- CSR: X[rows_na, ] <- NA_real_, then X[, cols_na] <- NA_real_
    dp, dj, dx = dev(p), dev(j), dev(x)
    ws = torch.empty(lib.mxd_gather_workspace_bytes(m), dtype=torch.uint8, device="cuda")
    cap = nnz + 1000 * n + 16 * m

    all_rows, all_cols = axis_of(None, m), axis_of(None, n)

    def assign(src, src_nnz, rows_axis, cols_axis, dst):
        sp, sj, sx = src
        np_, nj, nx = dst
        (ai, ni, _, _), (aj, nj_sel, _, sorted_j) = rows_axis, cols_axis
        total, hits = C.c_int64(0), C.c_int64(0)
        avg = src_nnz / m
        _lib.check(lib.mxd_csr_assign_count(m, n, vp(sp), vp(sj), src_nnz, C.byref(ai), C.byref(aj), ni, nj_sel, 1, avg,
                                            vp(np_), vp(ws), C.byref(total), C.byref(hits), stream))
        assert total.value <= cap
        _lib.check(lib.mxd_csr_assign_fill(m, n, vp(sp), vp(sj), vp(sx), C.byref(ai), C.byref(aj), vp(sorted_j), nj_sel,
                                           1, float(NA_REAL), avg, vp(np_), vp(nj), vp(nx), stream))
        return int(total.value)

    def bufs():
        return (torch.empty(m + 1, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"),
                torch.empty(cap, dtype=torch.float64, device="cuda"))
    first, second = bufs(), bufs()
    for name, rna, cna in cases:
        state = {}
        rows_axis = axis_of(rna, m) if rna.size else None     # the selector maps are made once, outside the timing
        cols_axis = axis_of(cna, n) if cna.size else None

        def run():
            src, k = (dp, dj, dx), nnz
            if rows_axis:
                k = assign(src, k, rows_axis, all_cols, first)
                src = first
            if cols_axis:
                k = assign(src, k, all_rows, cols_axis, second)
            state["total"] = k
        med, best = timed(run, a.warmup, a.iters)
        total = state["total"]
        nbytes = 4 * (m + 1) + 12 * total
        cmed, cbest = copy_of(nbytes, a.warmup, a.iters)
        report(dict(route="CSR", case=name, median_ms=round(med, 4), min_ms=round(best, 4), out_entries=total,
                    out_MB=round(nbytes / 1e6, 1), copy_median_ms=round(cmed, 4), copy_min_ms=round(cbest, 4),
                    times_the_copy=round(med / cmed, 2)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
