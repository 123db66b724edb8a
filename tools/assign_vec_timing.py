#!/usr/bin/env python3
"""Device-event timing of the vector-valued CSR assignment kernels (mxd_csr_assign_col_count + _fill,
mxd_csr_expand_pattern_row + mxd_csr_replace_rows_count + _fill) on device-resident operands: 5
warm-up runs, then 20 timed runs, median and min.

Input: cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32 M f64 entries), taken as a matrix of 100 001 columns so
that its last column c is stored by no row.  Four calls:
  X[, c] <- dense vector of 1 000 000 values, no row storing c       (every row grows by one entry)
  the same on that call's result, where every row stores c           (values only: no indices are written)
  X[, c] <- sparseVector of length 1 000 000 storing half the rows   (a binary search per row, half the rows grow)
  X[r, ] <- dense vector of 100 001 values                           (pattern expansion, then the row replacement)
Each call is timed next to a device-to-device copy of as many bytes as its output holds (indptr, indices, values; the
values alone for the second call): an operation that rewrites the matrix cannot be faster than that copy, so the ratio
says how far from the floor it is.  The timed region holds the count pass's host read-back.  No threshold is set: the
tool reports.

usage: python tools/assign_vec_timing.py [--warmup 5] [--iters 20] [--json out.json]
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
    ncols, col = n + 1, n
    assert int(j.max()) < col
    dp, dj, dx = dev(p), dev(j), dev(x)
    rng = np.random.default_rng(5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.mxd_gather_workspace_bytes(m), dtype=torch.uint8, device="cuda")
    new_p = torch.empty(m + 1, dtype=torch.int32, device="cuda")
    cap = nnz + ncols + m
    new_j = torch.empty(cap, dtype=torch.int32, device="cuda")
    new_x = torch.empty(cap, dtype=torch.float64, device="cuda")
    avg = nnz / m
    out = []

    def report(name, total, changed, nbytes, med, best):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        cmed, cbest = timed(lambda: dst.copy_(src), a.warmup, a.iters)
        res = dict(case=name, median_ms=round(med, 4), min_ms=round(best, 4), out_entries=total, rows_changed=changed,
                   out_MB=round(nbytes / 1e6, 1), copy_median_ms=round(cmed, 4), copy_min_ms=round(cbest, 4),
                   times_the_copy=round(med / cmed, 2))
        print(json.dumps(res), flush=True)
        out.append(res)

    def col_case(name, sp, sj, sx, s_nnz, ii, xx, values_only=False):
        total, changed = C.c_int64(0), C.c_int64(0)
        n_xx = int(xx.numel())
        s_avg = s_nnz / m

        def run():
            _lib.check(lib.mxd_csr_assign_col_count(m, ncols, vp(sp), vp(sj), s_nnz, col, vp(ii), n_xx, m, s_avg,
                                                    vp(new_p), vp(ws), C.byref(total), C.byref(changed), stream))
            assert total.value <= cap and (not values_only or changed.value == 0)
            _lib.check(lib.mxd_csr_assign_col_fill(m, ncols, vp(sp), vp(sj), vp(sx), col, vp(ii), vp(xx), n_xx, m, s_avg,
                                                   vp(sp) if values_only else vp(new_p),
                                                   None if values_only else vp(new_j), vp(new_x), stream))
        med, best = timed(run, a.warmup, a.iters)
        nbytes = 8 * total.value if values_only else 4 * (m + 1) + 12 * total.value
        report(name, int(total.value), int(changed.value), nbytes, med, best)
        return int(total.value)

    vec = dev(rng.normal(size=m))
    total = col_case("X[, c] <- dense vector, no row stores c", dp, dj, dx, nnz, None, vec)
    assert total == nnz + m
    fp, fj, fx = new_p.clone(), new_j[:total].clone(), new_x[:total].clone()
    col_case("X[, c] <- dense vector, every row stores c (values only)", fp, fj, fx, total, None, vec, values_only=True)
    half = np.sort(rng.choice(m, size=m // 2, replace=False)).astype(np.int32)
    col_case("X[, c] <- sparseVector storing half the rows", dp, dj, dx, nnz, dev(half), dev(rng.normal(size=half.size)))

    rowvec = dev(rng.normal(size=ncols))
    vptr = torch.empty(2, dtype=torch.int32, device="cuda")
    vj = torch.empty(ncols, dtype=torch.int32, device="cuda")
    vx = torch.empty(ncols, dtype=torch.float64, device="cuda")
    row = m // 2
    ai = _lib.CooAxis(_lib.MX_AXIS_AFFINE, row, row, 0, 0, None, None)
    total = C.c_int64(0)
    r_avg = (nnz + ncols) / m

    def row_case():
        _lib.check(lib.mxd_csr_expand_pattern_row(None, vp(rowvec), ncols, ncols, 1, vp(vptr), vp(vj), vp(vx), stream))
        _lib.check(lib.mxd_csr_replace_rows_count(m, vp(dp), C.byref(ai), 1, vp(vptr), vp(new_p), vp(ws),
                                                  C.byref(total), stream))
        assert total.value <= cap
        _lib.check(lib.mxd_csr_replace_rows_fill(m, vp(dp), vp(dj), vp(dx), C.byref(ai), 1, vp(vptr), vp(vj), vp(vx),
                                                 r_avg, vp(new_p), vp(new_j), vp(new_x), stream))
    med, best = timed(row_case, a.warmup, a.iters)
    report("X[r, ] <- dense vector", int(total.value), 1, 4 * (m + 1) + 12 * total.value, med, best)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
