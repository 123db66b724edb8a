#!/usr/bin/env python3
"""Device-event timing of the one-triangle Gram product next to the full product it replaces: 5 warm-up
runs, then 20 timed runs, median and min, the count pass and the fill pass apart.

  (b) crossprod   crossprod(X) for X = csr_fixed(1_000_000, 2_000, 8): case (b) of tools/spgemm_timing.py, 64 M products,
                  an almost dense 2_000 x 2_000 result, every row of the full product in the dense bin
  (c) tcrossprod  tcrossprod(X) for X = csr_fixed(200_000, 100_000, 16): some 100 M products on a sparse
                  200_000 x 200_000 result, short rows

For each case, on the cached column order (X.transposed()):
  full          mxd_csr_spgemm_count / _fill, and device.spgemm as it stands
  tri, sorted   mxd_csr_spgemm_tri_count / _fill with uplo U and b_sorted = 1 (both right-hand sides here are sorted), and
                device.spgemm(..., uplo="U")
  tri, as is    the same with b_sorted = 0: the keep rule alone, nothing trimmed
  expand        device.csr_symmetric_to_general of the triangle: what a caller who needs the general form pays on top
Each pass is set next to a device-to-device copy of the bytes it reads plus writes (`moved_MB`: every product the
bounds pass counted reads one index of B, and in the fill one value; the result is written once).

usage: python tools/gram_timing.py [--warmup 5] [--iters 20] [--json profiles/gram_timing.json] [--scale 1.0]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from matrixextra_amd import _lib, synth  # noqa: E402
from matrixextra_amd import device as D  # noqa: E402
from tools.spgemm_timing import copy_of, timed  # noqa: E402


def passes(A, B, mask):
    """(count, fill factory) of one product; mask: () for the full product, (uplo, b_sorted) for a triangle"""
    dev, dp = A.indptr.device, D._dp
    tri = "_tri" if mask else ""
    ws = D._workspace(dev, "mxd_csr_spgemm_workspace_bytes", A.m, B.K)
    out_p = D._int32(dev, A.m + 1)

    def count():
        return D._call(f"mxd_csr_spgemm{tri}_count", A.m, A.K, B.K, dp(A.indptr), dp(A.indices), A.nnz, dp(B.indptr),
                       dp(B.indices), B.nnz, *mask, dp(out_p), dp(ws), cells=D._COUNT * 2)

    def fill_into(out_j, out_x):
        return lambda: D._call(f"mxd_csr_spgemm{tri}_fill", A.m, A.K, B.K, dp(A.indptr), dp(A.indices), dp(A.values),
                               D._value_dtype(A.values), dp(B.indptr), dp(B.indices), dp(B.values),
                               D._value_dtype(B.values), *mask, dp(out_p), dp(out_j), dp(out_x), dp(ws))
    return count, fill_into, ws


def time_case(name, A, B, warmup, iters, out, save):
    dev = A.indptr.device
    assert B.rows_sorted()
    U = _lib.MX_UPLO_UPPER
    variants = (("full", (), lambda: D.spgemm(A, B)), ("tri, sorted", (U, 1), lambda: D.spgemm(A, B, uplo="U")),
                ("tri, as is", (U, 0), None))

    def emit(res):
        print(json.dumps(res), flush=True)
        out.append(res)
        save()

    for label, mask, whole in variants:
        count, fill_into, ws = passes(A, B, mask)
        products, nnz_out = count()
        out_j, out_x = D._entries(dev, nnz_out, torch.int32, torch.float64)
        base = dict(case=name, variant=label, m=A.m, K=A.K, n=B.K, nnzA=A.nnz, nnzB=B.nnz, products=products,
                    nnz_out=nnz_out, workspace_MB=round(ws.numel() / 1e6, 1))
        moved = {"count": 8 * (A.m + 1) + 12 * A.nnz + 4 * products,
                 "fill": 8 * (A.m + 1) + 20 * A.nnz + 12 * products + 12 * nnz_out}
        for what, fn in (("count", count), ("fill", fill_into(out_j, out_x))):
            med, best = timed(fn, warmup, iters)
            cmed, cbest = copy_of(moved[what], warmup, iters)
            emit(dict(base, what=what, median_ms=med, min_ms=best, moved_MB=round(moved[what] / 1e6, 1),
                      copy_median_ms=cmed, copy_min_ms=cbest))
        if whole is not None:
            med, best = timed(whole, warmup, iters)
            emit(dict(base, what="device.spgemm (workspace, count, allocation, fill)", median_ms=med, min_ms=best))
        del out_j, out_x, ws
    tri = D.spgemm(A, B, uplo="U")
    med, best = timed(lambda: D.csr_symmetric_to_general(tri, "U"), warmup, iters)
    emit(dict(case=name, variant="expand", what="device.csr_symmetric_to_general of the triangle", nnz_in=tri.nnz,
              nnz_out=D.csr_symmetric_to_general(tri, "U").nnz, median_ms=med, min_ms=best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the row counts of both cases (a trial run)")
    a = ap.parse_args()
    print("device:", _lib.device_name(), flush=True)
    out = []

    def save():
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)

    X = D.DeviceCSR.from_host(*synth.csr_fixed(int(1_000_000 * a.scale), 2_000, 8), 2_000)
    time_case("b: crossprod(X), X = csr_fixed(1M, 2k, 8)", X.transposed(), X, a.warmup, a.iters, out, save)
    del X
    X = D.DeviceCSR.from_host(*synth.csr_fixed(int(200_000 * a.scale), 100_000, 16), 100_000)
    time_case("c: tcrossprod(X), X = csr_fixed(200k, 100k, 16)", X, X.transposed(), a.warmup, a.iters, out, save)


if __name__ == "__main__":
    main()
