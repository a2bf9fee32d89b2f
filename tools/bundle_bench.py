#!/usr/bin/env python3
"""Times sdvl_bundle_adjust alone: J = 1, 16 and 256 problems of the `full` shape of tests/bundle_cases.py (11 free + 5 fixed
keyframes, 300 points, 1530 edges; 5 + 3 iterations) in one call.  Prints the kernel's dispatch time (HIP events around the launch)
and the wall time of the C call (index building, staging, launch, copy back) per J.
    python tools/bundle_bench.py [reps]"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundle_cases as bc  # noqa: E402

sdvl = importlib.import_module("slam-sdvl_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ctx = sdvl.Context(0)
full = bc.case("full")
for J in (1, 16, 256):
    probs = [full] * J
    out = ctx.bundle_adjust(probs, bc.CAM)          # warm-up: buffers grow here
    assert all(o["status"] == 0 for o in out)
    ctx.timing_enable(True)
    ctx.timing_only("bundle_adjust")
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.bundle_adjust(probs, bc.CAM)
    wall = (time.perf_counter() - t0) / reps * 1e3
    ms, launches = ctx.timing_get()["bundle_adjust"]
    ctx.timing_enable(False)
    trials = out[0]["stages"][0]["trials"] + out[0]["stages"][1]["trials"]
    print("J = %3d: kernel %.3f ms per call (%.1f us per problem, %d LM trials each), python call %.1f ms" % (J, ms / launches, ms / launches / J * 1e3, trials, wall))
ctx.close()
