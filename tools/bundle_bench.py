#!/usr/bin/env python3
"""Times sdvl_bundle_adjust alone: J = 1, 16 and 256 problems of the `full` shape of tests/bundle_cases.py (11 free + 5 fixed
keyframes, 300 points, 1530 edges; 5 + 3 iterations) in one call.  Prints the kernel's dispatch time (HIP events around the launch)
and the wall time of the C call (index building, staging, launch, copy back) per J.
--depth times the depth form (sdvl_bundle_adjust_depth) beside it: the same shape with a measured depth on every edge
(tests/bundle_depth_cases.py, `full/all`).
    python tools/bundle_bench.py [reps] [--depth]"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundle_cases as bc  # noqa: E402

sdvl = importlib.import_module("slam-sdvl_amd")
args = [a for a in sys.argv[1:] if a != "--depth"]
with_depth = "--depth" in sys.argv[1:]
reps = int(args[0]) if args else 5
ctx = sdvl.Context(0)
full = bc.case("full")
calls = [("monocular", "bundle_adjust", full, None)]
if with_depth:
    import bundle_depth_cases as dc  # noqa: E402
    calls.append(("depth on every edge", "bundle_adjust_depth", dc.case("full/all"), dc.BF))
for J in (1, 16, 256):
    for what, kernel, prob, bf in calls:
        probs = [prob] * J
        out = ctx.bundle_adjust(probs, bc.CAM, bf)      # warm-up: buffers grow here
        assert all(o["status"] == 0 for o in out)
        ctx.timing_enable(True)
        ctx.timing_only(kernel)
        ctx.timing_reset()
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.bundle_adjust(probs, bc.CAM, bf)
        wall = (time.perf_counter() - t0) / reps * 1e3
        ms, launches = ctx.timing_get()[kernel]
        ctx.timing_enable(False)
        trials = out[0]["stages"][0]["trials"] + out[0]["stages"][1]["trials"]
        print("J = %3d, %s: kernel %.3f ms per call (%.1f us per problem, %d LM trials each), python call %.1f ms"
              % (J, what, ms / launches, ms / launches / J * 1e3, trials, wall))
ctx.close()
