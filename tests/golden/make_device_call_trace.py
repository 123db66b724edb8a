#!/usr/bin/env python3
"""Writes tests/golden/device_call_trace.json: what matrixextra_amd/device.py does with its operands, function by
function, over the recording fake of libmxgpu.so in tests/device_trace.py (CPU tensors; neither the library nor a
device is needed): every library call with its arguments, every allocation, the shape and aliasing of every result,
and in a second table the type and message of every refusal.

The record was taken ONCE, from device.py as it stood at the commit named in the file ("taken_from"), before its
functions were rewritten on shared helpers, and is what tests/test_device_trace_host.py holds every later device.py to.
Do not regenerate it from the code under test.  A new wrapper, or a refusal added on purpose, is recorded when it is
added and left alone afterwards: run with the names of its cases, and only those entries are written.

    python tests/golden/make_device_call_trace.py [case or refusal name ...]
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import device_trace as T  # noqa: E402

OUT = os.path.join(HERE, "device_call_trace.json")


def write(record):
    def table(entries):                                    # one line per case, sorted: a change shows as that line
        return "{\n" + ",\n".join("%s: %s" % (json.dumps(n), json.dumps(entries[n], sort_keys=True))
                                  for n in sorted(entries)) + "\n}"
    with open(OUT, "w") as f:
        f.write('{"taken_from": %s,\n"cases": %s,\n"refusals": %s}\n'
                % (json.dumps(record["taken_from"]), table(record["cases"]), table(record["refusals"])))


def main(only):
    cases, refusals = T.cases(), T.refusals()
    if only:
        with open(OUT) as f:
            record = json.load(f)
        unknown = [n for n in only if n not in cases and n not in refusals]
        if unknown:
            sys.exit(f"no such case or refusal: {unknown}")
    else:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True)
        record = {"taken_from": head.stdout.strip(), "cases": {}, "refusals": {}}
    for name, case in cases.items():
        if not only or name in only:
            record["cases"][name] = T.run_case(case)
    for name, case in refusals.items():
        if not only or name in only:
            got = T.run_refusal(case)
            if got["type"] is None:
                print(f"NOT RECORDED, nothing is raised: {name}")
            else:
                record["refusals"][name] = got
    write(record)
    print(f"{OUT}: {len(record['cases'])} cases, {len(record['refusals'])} refusals, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
