#!/usr/bin/env python3
"""Timing of the export-level row concat (mx_concat_csr_batch_begin + mx_result_finish, what exports.concat_csr_batch
runs) on this tree's libmxgpu.so and, with --parent-lib, on another build of it (the parent commit's), alternated:
each version runs in --rounds fresh child processes, parent, this, parent, this, ..., so that the rounds of one version
give the run-to-run spread that a difference between the versions has to exceed.

Cases, all on cfg2's CSR, synth.csr_fixed(1_000_000, 100_000, 32) (32 M f64 entries):
  a  two halves of it                          (2 operands: the upload of 2 x 192 MB dominates)
  b  10 000 sparse vectors of 32 entries       (its first 10 000 rows as dsparseVectors; 320 000 entries out)
  c  1 000 matrices of 1 000 rows              (the whole of it in 1 000 blocks)
The call is synchronous for the host; it is timed with device events on the stream it uses (the null stream), 1 warm-up
run and --iters timed runs, median and min.  Beside each case: a device-to-device copy of as many bytes as the output
holds (indptr, indices, values), the floor of the device part.  A digest of the three output vectors is compared
between the versions: the results must be bit-identical.  No threshold is set: the tool reports.

usage: python tools/bind_timing.py [--parent-lib other/libmxgpu.so] [--iters 5] [--rounds 2]
                                   [--json profiles/bind_timing.json]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(lib_path, iters):
    import numpy as np
    import torch

    from matrixextra_amd import _lib, synth

    lib = C.CDLL(lib_path)                                  # this version only: nothing else of the package is loaded
    for name in ("mx_concat_csr_batch_begin", "mx_result_finish", "mx_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HEADER.functions[name]

    def check(rc):
        if rc:
            raise RuntimeError(lib.mx_last_error().decode())

    m, n, per_row = 1_000_000, 100_000, 32
    p, j, x = synth.csr_fixed(m, n, per_row)

    def block(r0, r1):
        return (0, np.ascontiguousarray(p[r0:r1 + 1] - p[r0]), j[p[r0]:p[r1]], x[p[r0]:p[r1]], r1 - r0)

    cases = {
        "a_two_halves_of_cfg2": [block(0, m // 2), block(m // 2, m)],
        "b_10000_vectors_of_32": [(3, None, j[p[r]:p[r + 1]] + 1, x[p[r]:p[r + 1]], 1) for r in range(10_000)],
        "c_1000_matrices_of_1000_rows": [block(r, r + 1000) for r in range(0, m, 1000)],
    }

    def timed(run, warmup, k):
        for _ in range(warmup):
            run()
        times = []
        for _ in range(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times)), float(np.min(times))

    for name, objs in cases.items():
        arr = (_lib.RbindInput * len(objs))()
        for k, (kind, pp, jj, xx, nr) in enumerate(objs):
            arr[k] = _lib.RbindInput(kind, None if pp is None else pp.ctypes.data, jj.ctypes.data, xx.ctypes.data, nr,
                                     jj.size)
        nrows, nnz = sum(o[4] for o in objs), sum(o[2].size for o in objs)
        op, oj, ox = np.empty(nrows + 1, np.int32), np.empty(nnz, np.int32), np.empty(nnz, np.float64)

        def run():
            res, info = C.c_void_p(), _lib.ResultInfo()
            check(lib.mx_concat_csr_batch_begin(arr, len(objs), 0, C.byref(res), C.byref(info)))
            assert (info.indptr_len, info.nnz, info.values_len) == (nrows + 1, nnz, nnz)
            check(lib.mx_result_finish(res, op.ctypes.data, oj.ctypes.data, ox.ctypes.data))

        med, best = timed(run, 1, iters)
        digest = hashlib.sha256(op.tobytes() + oj.tobytes() + ox.tobytes()).hexdigest()[:16]
        nbytes = op.nbytes + oj.nbytes + ox.nbytes
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        cmed, cbest = timed(lambda: dst.copy_(src), 3, 10)
        print(json.dumps(dict(case=name, operands=len(objs), out_rows=nrows, out_entries=nnz, out_MB=round(nbytes / 1e6, 1),
                              median_ms=round(med, 3), min_ms=round(best, 3), copy_median_ms=round(cmed, 4),
                              copy_min_ms=round(cbest, 4), digest=digest)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per version")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters)
    this = os.path.join(ROOT, "matrixextra_amd", "libmxgpu.so")
    rounds = ([("parent", a.parent_lib), ("this", this)] if a.parent_lib else [("this", this)]) * a.rounds
    runs = []
    for version, path in rounds:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", os.path.abspath(path), "--iters",
                              str(a.iters)], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.exit(f"{version} ({path}) failed with status {out.returncode}:\n{out.stderr[-2000:]}")
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                runs.append(dict(version=version, **json.loads(line)))
                print(json.dumps(runs[-1]), flush=True)
    summary = []
    for case in dict.fromkeys(r["case"] for r in runs):
        of = {v: [r for r in runs if r["case"] == case and r["version"] == v] for v in ("parent", "this")}
        assert len({r["digest"] for r in runs if r["case"] == case}) == 1, f"{case}: the versions' results differ"
        row = dict(case=case, **{k: of["this"][0][k] for k in ("operands", "out_rows", "out_entries", "out_MB")})
        for v, rs in of.items():
            if rs:
                meds = [r["median_ms"] for r in rs]
                row[v + "_median_ms"] = meds
                row[v + "_min_ms"] = min(r["min_ms"] for r in rs)
                row[v + "_spread"] = round(max(meds) / min(meds) - 1, 4)
        if of["parent"]:
            row["parent_over_this"] = round(min(row["parent_median_ms"]) / min(row["this_median_ms"]), 2)
        row["copy_median_ms"] = of["this"][0]["copy_median_ms"]
        summary.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(runs=runs, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
