"""The job lists of the device calls that read a frame's depth image or right image, without a GPU: host/depth_jobs.h makes them for
SDVLBatch (host/batch_depth.cc) and includes nothing of the device layer beyond the C-ABI's structs.  `make depth_jobs_check` builds
host/depth_jobs_check.cc, which drives the builder with fake DepthImage headers over dummy pointers.  It checks that the ranges are
contiguous and in call order, that an owner without an image gets no job, that a job carries its image's fields (and a stereo job the
left frame and the stride), and that the builder refuses unequal depth rules, unequal stereo rules, a right image offered as a depth
image, a depth image offered as a right image, and both producers in one call."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slam-sdvl_amd", "host")


def test_depth_jobs_header_stays_off_the_device_layer():
    includes = re.findall(r'#include\s+([<"][^>"]+[>"])', open(os.path.join(HOST, "depth_jobs.h")).read())
    assert [i for i in includes if i.startswith('"')] == ['"../../include/sdvl_hip.h"', '"types.h"'], includes
    includes = re.findall(r'#include\s+([<"][^>"]+[>"])', open(os.path.join(HOST, "depth_jobs_check.cc")).read())
    assert [i for i in includes if i.startswith('"')] == ['"depth_jobs.h"'], includes
    rule = open(os.path.join(HOST, "Makefile")).read().split("\ndepth_jobs_check:", 1)[1].split("\n\n", 1)[0]
    assert "-lsdvl" not in rule and "libsdvl" not in rule, rule


def test_depth_jobs_check_program_passes():
    subprocess.run(["make", "-s", "-C", HOST, "depth_jobs_check"], check=True)
    out = subprocess.run([os.path.join(HOST, "depth_jobs_check")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "depth_jobs_check: ok" in out.stdout, out.stdout + out.stderr
