#!/usr/bin/env python3
"""Device-event timing of the sparse x sparse product: 5 warm-up runs, then 20 timed runs, median and
min, the count pass and the fill pass apart.

  (a) product    csr_fixed(200_000, 100_000, 16) %*% csr_fixed(100_000, 100_000, 16): 51.2 M products, short rows of B
  (b) crossprod  crossprod(X) for X = csr_fixed(1_000_000, 2_000, 8) through the cached column order (X.transposed()):
                 64 M products, an almost dense 2_000 x 2_000 result, every row in the dense bin

Each pass is set next to a device-to-device copy of the bytes it reads plus writes (`moved_MB`; every product reads one
index of B, and in the fill one value, and the result is written once), and the whole product next to torch.sparse.mm
of the same operands as sparse_csr tensors; if this torch build refuses that, the refusal is recorded instead.

usage: python tools/spgemm_timing.py [--warmup 5] [--iters 20] [--json profiles/spgemm_timing.json] [--scale 1.0]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matrixextra_amd import _lib, synth  # noqa: E402
from matrixextra_amd import device as D  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 4), round(float(np.min(times)), 4)


def copy_of(nbytes, warmup, iters):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), warmup, iters)


def torch_csr(A):
    return torch.sparse_csr_tensor(A.indptr, A.indices, A.values, size=(A.m, A.K))


def time_product(name, A, B, warmup, iters, out, save):
    dev = A.indptr.device
    dp = D._dp
    ws = D._workspace(dev, "mxd_csr_spgemm_workspace_bytes", A.m, B.K)
    out_p = D._int32(dev, A.m + 1)

    def count():
        return D._call("mxd_csr_spgemm_count", A.m, A.K, B.K, dp(A.indptr), dp(A.indices), A.nnz, dp(B.indptr),
                       dp(B.indices), B.nnz, dp(out_p), dp(ws), cells=D._COUNT * 2)

    products, nnz_out = count()
    out_j, out_x = D._entries(dev, nnz_out, torch.int32, torch.float64)

    def fill():
        D._call("mxd_csr_spgemm_fill", A.m, A.K, B.K, dp(A.indptr), dp(A.indices), dp(A.values), D._value_dtype(A.values),
                dp(B.indptr), dp(B.indices), dp(B.values), D._value_dtype(B.values), dp(out_p), dp(out_j), dp(out_x), dp(ws))

    limits = [D.C.c_int(0) for _ in range(3)]
    _lib.check(_lib.load().mxd_csr_spgemm_limits(A.m, B.K, *map(D.C.byref, limits)))
    base = dict(case=name, m=A.m, K=A.K, n=B.K, nnzA=A.nnz, nnzB=B.nnz, products=products, nnz_out=nnz_out,
                group_ub=limits[0].value, lds_ub=limits[1].value, dense_groups=limits[2].value,
                workspace_MB=round(ws.numel() / 1e6, 1))
    moved = {"count": 8 * (A.m + 1) + 12 * A.nnz + 4 * products,
             "fill": 8 * (A.m + 1) + 20 * A.nnz + 12 * products + 12 * nnz_out}
    for what, fn in (("count", count), ("fill", fill)):
        med, best = timed(fn, warmup, iters)
        cmed, cbest = copy_of(moved[what], warmup, iters)
        res = dict(base, what=what, median_ms=med, min_ms=best, moved_MB=round(moved[what] / 1e6, 1), copy_median_ms=cmed,
                   copy_min_ms=cbest, products_per_ns=round(products / med / 1e6, 3))
        print(json.dumps(res), flush=True)
        out.append(res)
        save()
    med, best = timed(lambda: D.spgemm(A, B), warmup, iters)
    res = dict(base, what="spgemm (workspace, count, allocation, fill)", median_ms=med, min_ms=best)
    try:                                    # the same product by torch, on sparse_csr tensors
        ta, tb = torch_csr(A), torch_csr(B)
        C = torch.sparse.mm(ta, tb)
        res["torch_nnz"] = int(C.values().numel())
        del C
        tmed, tbest = timed(lambda: torch.sparse.mm(ta, tb), warmup, iters)
        res.update(torch_sparse_mm_median_ms=tmed, torch_sparse_mm_min_ms=tbest)
    except Exception as e:                  # noqa: BLE001 - whatever this build says is the record
        res["torch_sparse_mm_refused"] = f"{type(e).__name__}: {str(e)[:300]}"
    print(json.dumps(res), flush=True)
    out.append(res)
    save()


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

    m = int(200_000 * a.scale)
    A = D.DeviceCSR.from_host(*synth.csr_fixed(m, 100_000, 16), 100_000)
    B = D.DeviceCSR.from_host(*synth.csr_fixed(100_000, 100_000, 16, seed=7), 100_000)
    time_product("a: csr_fixed(200k, 100k, 16) %*% csr_fixed(100k, 100k, 16)", A, B, a.warmup, a.iters, out, save)
    del A, B
    X = D.DeviceCSR.from_host(*synth.csr_fixed(int(1_000_000 * a.scale), 2_000, 8), 2_000)
    med, best = timed(lambda: X.transposed(), a.warmup, a.iters)
    out.append(dict(case="b", what="X.transposed() on the cached order", median_ms=med, min_ms=best))
    print(json.dumps(out[-1]), flush=True)
    time_product("b: crossprod(X), X = csr_fixed(1M, 2k, 8)", X.transposed(), X, a.warmup, a.iters, out, save)


if __name__ == "__main__":
    main()
