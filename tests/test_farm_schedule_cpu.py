"""The farm's scheduling without a GPU: host/farm_schedule.h holds everything the worker threads, the fibers and the feeder thread of a
TrackerFarm run share, and includes nothing of the device layer.  `make farm_schedule_check` builds host/farm_schedule_check.cc, which
drives it the way host/farm.cc does, with fake group-steps (short pseudo-random sleeps): owned and dynamic runs, a host-fed run with a
feeder thread and rings of three slots, a failing group-step, and the non-blocking calls from one thread.  It checks that every group
runs its steps in order and once, that no two threads are inside one group, that the feeder never runs a ring's length ahead and always
serves the group that is furthest behind, and that the first failure ends the run and is the one reported."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slam-sdvl_amd", "host")


def test_schedule_header_is_standard_library_only():
    for name in ("farm_schedule.h", "farm_schedule_check.cc"):
        includes = re.findall(r'#include\s+([<"][^>"]+[>"])', open(os.path.join(HOST, name)).read())
        ours = [i for i in includes if i.startswith('"')]
        assert ours == ([] if name == "farm_schedule.h" else ['"farm_schedule.h"']), (name, ours)
        assert not [i for i in includes if "hip" in i or "sdvl_host" in i], (name, includes)
    rule = open(os.path.join(HOST, "Makefile")).read().split("\nfarm_schedule_check:", 1)[1].split("\n\n", 1)[0]
    assert "-lsdvl" not in rule and "libsdvl" not in rule, rule


def test_schedule_check_program_passes():
    subprocess.run(["make", "-s", "-C", HOST, "farm_schedule_check"], check=True)
    out = subprocess.run([os.path.join(HOST, "farm_schedule_check")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "farm_schedule_check: ok" in out.stdout, out.stdout + out.stderr
