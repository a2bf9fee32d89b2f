"""sdvl_depth_lookup (include/sdvl_hip.h) restated: depth seeding's rule at positions of the caller's own.  It is composed of what is
already stated and not edited: depth_seed_restatement (validity of a sample, status codes, the rule's defaults, metres of a 16-bit sample)
and depth_measure_restatement.lookup, the same lookup as the measured depth filter makes it at a found pixel.

  position   px, a level-0 position of the gray image (sub-pixel), and the pyramid level the feature was found on
  centre     floor(px + 0.5); with a lens of the raw pixel px's ray lands on
  window     nine samples at stride 1 << level around the centre
  status, z  OUTSIDE, HOLE, FEW, EDGE in that order, else OK and z = the centre sample in metres; z = 0 unless OK
  jobs       (depth image, begin, end[, scale]): the positions begin .. end belong to that image; a position in no job is HOLE

Test infrastructure only."""
import numpy as np

import depth_measure_restatement as dmr
import depth_seed_restatement as dsr
from depth_seed_restatement import EDGE, FEW, HOLE, OK, OUTSIDE  # noqa: F401


def depth_lookup(jobs, px, levels, cam, dist=None, **rule):
    """cam: dict(fx, fy, u0, v0) -> (z float64 [n], status uint8 [n], ok per job int32)"""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    n = len(px)
    z, status, ok = np.zeros(n), np.full(n, HOLE, np.uint8), np.zeros(len(jobs), np.int32)
    for j, job in enumerate(jobs):
        scale = float(job[3]) if len(job) > 3 else 1.0
        for i in range(int(job[1]), int(job[2])):
            status[i], z[i] = dmr.lookup(job[0], px[i], int(levels[i]), cam, dist, scale, rule)
            ok[j] += status[i] == OK
    return z, status, ok
