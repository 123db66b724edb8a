#!/usr/bin/env python3
"""Device-event timing of the dense <-> compressed conversions: 5 warm-up runs, then 20 timed runs,
median and min, both directions and both by_col values, on

  tall    a 1_000_000 x 128 float64 matrix with 1 %, 10 % and 50 % of its cells non-zero
  square  a 10_000 x 10_000 float64 matrix with 1 %

The matrices are column-major.  For dense -> compressed the count pass, the fill pass and device.dense_to_csr as a
whole (workspace, count, allocation, fill) are timed apart; for compressed -> dense the one launch of
mxd_csr_to_dense with a caller's flag (no read-back).  Each is set next to
  copy    a device-to-device copy of `moved_MB` bytes, the bytes the conversion must move once: 8 m n on the dense side
          plus 12 nnz + 4 (segments + 1) on the sparse side (the count pass: 8 m n alone).  As in the other timing tools
          the copy is dst.copy_(src) of that many bytes, so it reads and writes them: twice the traffic.
  torch   torch.Tensor.to_sparse_csr() / .to_dense() of the same matrix, for context (CSR only; int64 indices).

usage: python tools/dense_timing.py [--warmup 5] [--iters 20] [--json profiles/dense_timing.json] [--scale 1.0]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from matrixextra_amd import _lib  # noqa: E402
from matrixextra_amd import device as D  # noqa: E402
from tools.spgemm_timing import copy_of, timed  # noqa: E402


def make_dense(m, n, density, seed):
    """m x n float64, column-major, about `density` of the cells non-zero"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.rand((n, m), generator=g, device="cuda", dtype=torch.float64)
    X = torch.where(X < density, X + 1.0, torch.zeros_like(X))
    return X.t()


def time_case(name, m, n, density, warmup, iters, emit):
    X = make_dense(m, n, density, seed=m + n)
    dev, dp = X.device, D._dp
    assert X.stride() == (1, m)
    for by_col in (1, 0):
        nseg = n if by_col else m
        ws = D._workspace(dev, "mxd_dense_to_csr_workspace_bytes", m, n, by_col, 0)
        out_p = D._int32(dev, nseg + 1)

        def count():
            return D._call("mxd_dense_to_csr_count", m, n, dp(X), m, _lib.MX_F64, by_col, 0, dp(out_p), dp(ws), cells=D._COUNT)

        nnz, = count()
        out_j, out_x = D._entries(dev, nnz, torch.int32, torch.float64)

        def fill():
            return D._call("mxd_dense_to_csr_fill", m, n, dp(X), m, _lib.MX_F64, by_col, 0, dp(out_p), dp(ws), dp(out_j),
                           dp(out_x), _lib.MX_F64)

        dense_bytes, sparse_bytes = 8 * m * n, 12 * nnz + 4 * (nseg + 1)
        base = dict(case=name, m=m, n=n, density=density, by_col=by_col, nnz=nnz, workspace_MB=round(ws.numel() / 1e6, 2))
        for what, fn, moved in (("dense -> compressed: count", count, dense_bytes),
                                ("dense -> compressed: fill", fill, dense_bytes + sparse_bytes),
                                ("dense -> compressed: device.dense_to_csr", lambda: D.dense_to_csr(X, by_col=bool(by_col)),
                                 2 * dense_bytes + sparse_bytes)):
            med, best = timed(fn, warmup, iters)
            cmed, cbest = copy_of(moved, warmup, iters)
            emit(dict(base, what=what, median_ms=med, min_ms=best, moved_MB=round(moved / 1e6, 1), copy_median_ms=cmed,
                      copy_min_ms=cbest, ratio_to_copy=round(med / cmed, 2)))
        A = D.DeviceCSR(out_p, out_j[:nnz], out_x[:nnz], nseg, m if by_col else n, nnz, _sorted=True)
        out = torch.empty((n, m), dtype=torch.float64, device=dev).t()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        moved = dense_bytes + sparse_bytes
        med, best = timed(lambda: D.csr_to_dense(A, by_col=bool(by_col), out=out, flag=flag), warmup, iters)
        cmed, cbest = copy_of(moved, warmup, iters)
        assert int(flag.item()) == 0 and torch.equal(out, X)
        emit(dict(base, what="compressed -> dense: mxd_csr_to_dense", median_ms=med, min_ms=best,
                  moved_MB=round(moved / 1e6, 1), copy_median_ms=cmed, copy_min_ms=cbest, ratio_to_copy=round(med / cmed, 2)))
        del A, out, out_j, out_x, ws
    # torch, for context
    Xr = X.contiguous()                                                  # torch's conversions take the row-major matrix
    med, best = timed(lambda: Xr.to_sparse_csr(), warmup, iters)
    emit(dict(case=name, m=m, n=n, density=density, what="torch: to_sparse_csr()", median_ms=med, min_ms=best))
    S = Xr.to_sparse_csr()
    med, best = timed(lambda: S.to_dense(), warmup, iters)
    emit(dict(case=name, m=m, n=n, density=density, what="torch: to_dense()", median_ms=med, min_ms=best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the row counts of all cases (a trial run)")
    a = ap.parse_args()
    print("device:", _lib.device_name(), flush=True)
    out = []

    def emit(res):
        print(json.dumps(res), flush=True)
        out.append(res)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)

    for density in (0.01, 0.1, 0.5):
        time_case(f"tall: 1M x 128, {density:.0%}", int(1_000_000 * a.scale), 128, density, a.warmup, a.iters, emit)
    time_case("square: 10k x 10k, 1%", int(10_000 * a.scale), 10_000, 0.01, a.warmup, a.iters, emit)


if __name__ == "__main__":
    main()
