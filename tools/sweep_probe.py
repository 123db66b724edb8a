#!/usr/bin/env python3
"""Where the planned sweep's wavefronts wait (run on the GPU box):

    make -C matrixextra_amd/csrc PROBE=1 && python tools/sweep_probe.py [--lib PATH] [--out FILE]

Loads the probe build of the library (MX_SWEEP_PROBE in spmm_plan.hip), runs the headline product with a kept plan and
prints, per wavefront and launch: the time from the end of a batch of 8 steps to the completion of consume(0) of the
next batch, for batches without and with a panel meeting behind them, and the time from the end of a generation's
stream loop to the first consume(0) of the next generation that waits for a B line.  The meeting's cost is the
difference of the two batch figures times the number of meetings; the turnover's cost is its figure times the number
of turnovers (it contains the last batch's 8 consumes, the epilogue and the restart of the pipeline).
"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, ".")
import torch
from matrixextra_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(os.path.dirname(_lib.LIB_PATH), "libmxgpu_probe.so"))
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--panels", type=int, default=0)
args = ap.parse_args()
_lib.LIB_PATH = os.path.abspath(args.lib)
from matrixextra_amd import device as D, synth

lib = _lib.load()
m, K, n = 1_000_000, 100_000, 128
p, j, x = synth.csr_fixed(m, K, 32)
A = D.DeviceCSR.from_host(p, j, x, K)
B = torch.from_numpy(synth.dense_normal(K, n)).cuda()
out = torch.empty((n, m), dtype=torch.float64, device="cuda")
run = lambda: D.spmm_planned(A, B, out=out, colmajor=True, npanels=args.panels)
buf = (C.c_ulonglong * 64)()
for _ in range(2):
    run()
_lib.check(lib.mxd_spmm_sweep_probe(buf))                       # clears the warm-up's counts
_lib.check(lib.mxd_spmm_kernel_timing(1))
for _ in range(args.reps):
    run()
ms = (C.c_float * 64)()
cnt = C.c_int(0)
_lib.check(lib.mxd_spmm_kernel_times(ms, 64, C.byref(cnt)))
_lib.check(lib.mxd_spmm_kernel_timing(0))
_lib.check(lib.mxd_spmm_sweep_probe(buf))
tot = [sum(buf[8 * xcd + k] for xcd in range(8)) for k in range(8)]
waves = tot[6] / args.reps                                      # wavefronts per launch
kernel_ms = sum(ms[i] for i in range(cnt.value)) / max(cnt.value, 1)
TICK_US = 0.01                                                  # wall_clock64: 100 MHz
res = dict(lib=os.path.basename(args.lib), npanels=A.plan_info()["npanels"], kernel_ms_probe_build=round(kernel_ms, 4),
           wavefronts_per_launch=waves)
for k, name in enumerate(("batch_plain", "batch_after_meeting", "turnover")):
    s, c = tot[2 * k], tot[2 * k + 1]
    res[name] = dict(mean_us=round(s / max(c, 1) * TICK_US, 4), per_wave_per_launch=round(c / max(tot[6], 1), 2),
                     us_per_wave_per_launch=round(s / max(tot[6], 1) * TICK_US, 2))
excess = res["batch_after_meeting"]["mean_us"] - res["batch_plain"]["mean_us"]
res["meeting_excess_us_per_wave_per_launch"] = round(excess * res["batch_after_meeting"]["per_wave_per_launch"], 2)
res["meeting_excess_share_of_kernel"] = round(res["meeting_excess_us_per_wave_per_launch"] / (kernel_ms * 1e3), 4)
res["turnover_share_of_kernel"] = round(res["turnover"]["us_per_wave_per_launch"] / (kernel_ms * 1e3), 4)
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
