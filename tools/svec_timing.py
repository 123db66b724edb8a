#!/usr/bin/env python3
"""Device-event timing of RsparseMatrix * sparseVector (device.csr_by_svec) on device-resident
operands: 5 warm-up runs, then 20 timed runs, median, min and max.

Input: cfg2's matrix (1 M x 100 k, 32 entries per row, 32 M entries: 384 MB of indices and values) and a sparse vector
of length nrow that stores half of its positions.  Cases:
  finite       finite v, clean X, NAs kept (the default)
  ignore_na    the same under MatrixExtra.ignore_na
  dense-fill   0.01 % of the stored values NaN / Inf: those rows come out with all 100 k columns
  pair         the yardstick for `finite`: what the same result costs without this route, the device row gather of
               the stored rows (copy_csr_rows_numeric's passes) followed by the values-only mxd_csr_by_dvec over the
               gathered rows.  Its own spread, max / min over its runs, is the margin for the ratio of medians
               finite / pair.

Algorithmic bytes (m rows, nnz entries, nv stored positions, S = entries of the stored rows, U = entries of the
other rows, T = output entries):
  count   4 (m+1) indptr + 8 U (keep NAs: the values of the rows v does not store) + 4 m counts + 4 m positions
          in v; the scan 8 (m+1)
  fill    8 (m+1) both indptr + 4 m positions + 12 S read + 12 T written
  v       4 nv + 8 nv per pass (binary-searched; it stays in L2, counted once per pass)
  pair    gather: 4 r + 8 r + 4 (r+1) + 24 S; dvec: 4 (r+1) + 12 S + 8 r + 8 S
The share is against the ~6.3 TB/s achievable HBM rate.  The timings hold the count's host read-back (one
synchronise), so they are upper bounds on the kernels' time.

usage: python tools/svec_timing.py [--warmup 5] [--iters 20] [--json out.json]
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
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def report(name, alg, t, **extra):
    med, best, worst = t
    res = dict(case=name, median_ms=round(med, 4), min_ms=round(best, 4), max_ms=round(worst, 4),
               algorithmic_MB=round(alg / 1e6, 1), GBps_median=round(alg / med / 1e6, 1),
               hbm_share_median=round(alg / (med * 1e-3) / HBM_ACHIEVABLE, 3), **extra)
    print(json.dumps(res), flush=True)
    return res


def fused_bytes(m, nv, S, U, T, keep):
    count = 4 * (m + 1) + (8 * U if keep else 0) + 4 * m + 4 * m + 8 * (m + 1) + 12 * nv
    return count + 8 * (m + 1) + 4 * m + 12 * S + 12 * T + 12 * nv


def pair(A, rows, dvec):
    """gather of the stored rows, then the values-only product of the gathered rows with their values"""
    g = D.csr_gather_rows(A, rows)
    out = torch.empty(max(g.nnz, 1), dtype=torch.float64, device=rows.device)
    _lib.check(_lib.load().mxd_csr_by_dvec(g.m, g.K, g.nnz, D._dp(g.indptr), D._dp(g.indices), D._dp(g.values),
                                           D._dp(dvec), dvec.numel(), 0, 1, D._dp(out), D._stream()))
    return g, out


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
    nnz = j.size
    rng = np.random.default_rng(11)
    vi_h = (np.flatnonzero(rng.random(m) < 0.5) + 1).astype(np.int32)
    nv = vi_h.size
    vx_h = rng.uniform(0.5, 2.0, size=nv)
    vi, vx = torch.from_numpy(vi_h).cuda(), torch.from_numpy(vx_h).cuda()
    S, U = nv * per_row, (m - nv) * per_row
    out = []

    rp, rj, rx = D.csr_by_svec(A, vi, vx, m, keep_na=True)
    assert rj.numel() == S
    t_f = timed(lambda: D.csr_by_svec(A, vi, vx, m, keep_na=True), a.warmup, a.iters)
    fin = report("finite v, clean X, keep NAs", fused_bytes(m, nv, S, U, S, True), t_f, nnz=nnz, stored=nv,
                 out_entries=S)
    t_i = timed(lambda: D.csr_by_svec(A, vi, vx, m, keep_na=False), a.warmup, a.iters)
    out += [fin, report("finite v, clean X, ignore_na", fused_bytes(m, nv, S, U, S, False), t_i, nnz=nnz, stored=nv,
                        out_entries=S)]

    rows = (vi - 1).contiguous()
    g, gx = pair(A, rows, vx)
    torch.cuda.synchronize()
    assert torch.equal(g.indices, rj) and torch.equal(gx[:g.nnz], rx)
    del g, gx, rp, rj, rx
    t_p = timed(lambda: pair(A, rows, vx), a.warmup, a.iters)
    pair_bytes = 4 * nv + 8 * nv + 4 * (nv + 1) + 24 * S + 4 * (nv + 1) + 12 * S + 8 * nv + 8 * S
    pr = report("pair: row gather + values-only dvec (yardstick)", pair_bytes, t_p, nnz=nnz, stored=nv, out_entries=S)
    ratio, margin = t_f[0] / t_p[0], t_p[2] / t_p[1]
    verdict = dict(case="finite / pair", ratio_of_medians=round(ratio, 3), pair_spread_max_over_min=round(margin, 3),
                   within_margin=bool(ratio <= margin))
    print(json.dumps(verdict), flush=True)
    out += [pr, verdict]

    bad = rng.choice(nv, max(int(nv * 1e-4), 1), replace=False)
    vx_h2 = vx_h.copy()
    vx_h2[bad] = np.resize([np.nan, np.inf, -np.inf], bad.size)
    vx2 = torch.from_numpy(vx_h2).cuda()
    rp, rj, rx = D.csr_by_svec(A, vi, vx2, m, keep_na=True)
    T = rj.numel()
    del rp, rj, rx
    t_d = timed(lambda: D.csr_by_svec(A, vi, vx2, m, keep_na=True), a.warmup, a.iters)
    out.append(report("0.01 % of stored values NaN / Inf (dense-filled rows); no yardstick, unmeasured against anything",
                      fused_bytes(m, nv, S, U, T, True), t_d, nnz=nnz, stored=nv, dense_rows=int(bad.size),
                      out_entries=T))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
