#!/usr/bin/env python3
"""Generate the reference's data that tests/test_config_constants.py and tests/test_orb_pattern_pinned.py check against, so that
they run without the reference tree:

  reference_config/config_{tum_f1,tum_f2,euroc}.cfg   the reference's configuration files, byte for byte (config/)
  reference_orb.npz   bit_pattern_31: the 256 x 4 ORB sampling table parsed out of extra/orb_detector.cc by a parser of
                      its own (first_line: the line its first row is on); umax_lines: the line of each of UMAX_STATEMENTS,
                      the statements of the circular-patch row ends (orb_detector.cc:325-348), -1 where one is missing

    python tests/golden/make_reference_fixtures.py REFERENCE_TREE     # rewrites the fixtures (only when the reference changes)
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = ("config_tum_f1.cfg", "config_tum_f2.cfg", "config_euroc.cfg")
UMAX_STATEMENTS = ("int HALF_PATCH_SIZE = Config::ORBSize()/2;", "vmax = cvFloor(HALF_PATCH_SIZE * sqrt(2.f) / 2 + 1);",
                   "int vmin = cvCeil(HALF_PATCH_SIZE * sqrt(2.f) / 2);", "umax_[v] = cvRound(sqrt(hp2 - v * v));",
                   "while (umax_[v0] == umax_[v0 + 1])", "umax_[v] = v0;")


def orb_table(lines):
    start = next(i for i, l in enumerate(lines) if "bit_pattern_31_[256*4]" in l)
    nums = []
    for l in lines[start + 1:]:
        if l.strip().startswith("};"):
            break
        body = l.split("/*")[0]          # every row ends in a /*mean (...), correlation (...)*/ comment
        nums += [int(t) for t in body.split(",") if t.strip()]
    return start + 1, nums


def main(ref):
    cfg_dir = os.path.join(HERE, "reference_config")
    os.makedirs(cfg_dir, exist_ok=True)
    for name in CONFIGS:
        shutil.copyfile(os.path.join(ref, "config", name), os.path.join(cfg_dir, name))
    lines = open(os.path.join(ref, "extra", "orb_detector.cc")).read().splitlines()
    first_line, nums = orb_table(lines)
    umax_lines = [next((i + 1 for i, l in enumerate(lines) if s in l), -1) for s in UMAX_STATEMENTS]
    np.savez(os.path.join(HERE, "reference_orb.npz"), bit_pattern_31=np.array(nums, np.int8), first_line=np.int32(first_line),
             umax_lines=np.array(umax_lines, np.int32))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
