"""Designed inputs for the depth-seeding rule (tests/depth_seed_restatement.py), shared by the CPU test of the restatement and the GPU
tests of the device kernel: small depth images with a known answer, the `shelf` scene through a lens, and `shelf` frames with the
oracle's filtered corners.  Every case is dict(depth, xyl, cam, dist, scale, rule, want): `want` the statuses the case is designed for
(None where the restatement is the only statement).  Made once per process, read-only.

Test infrastructure only."""
import numpy as np

import depth_seed_restatement as dr
from oraclelib import TUM_CAM, TUM2_CAM, TUM2_DIST, trajectory_pose
import scene_cases as sc

_made = {}


def ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def case(depth, xyl, want=None, cam=TUM_CAM, dist=None, scale=1.0, **rule):
    return dict(depth=ro(depth), xyl=ro(np.asarray(xyl, np.int32).reshape(-1, 3)), cam=cam, dist=dist, scale=scale, rule=rule,
                want=None if want is None else np.asarray(want, np.uint8))


def plane_case():
    """a fronto-parallel plane at 1.5 m: every corner OK with exactly that depth"""
    rng = np.random.default_rng(20261001)
    depth = np.full((48, 64), 1.5, np.float32)
    l = rng.integers(0, 3, 40)
    x = rng.integers(2, (62 >> l) - 1)
    y = rng.integers(2, (46 >> l) - 1)
    return case(depth, np.stack([x, y, l], 1), np.zeros(40))


STEP_COLUMN = 30


def step_case(height):
    """a vertical depth step at column STEP_COLUMN: 2 m left of it, 2 (1 + height) m from it on.  Level-0 corners in columns 26 .. 34 of
    three rows: the window (columns cx - 1 .. cx + 1) straddles the step for cx = 29 and cx = 30 alone"""
    depth = np.full((48, 64), 2.0, np.float32)
    depth[:, STEP_COLUMN:] = np.float32(2.0 * (1.0 + height))
    xyl = [(x, y, 0) for y in (10, 20, 30) for x in range(26, 35)]
    straddle = [x in (STEP_COLUMN - 1, STEP_COLUMN) for x, _, _ in xyl]
    return case(depth, xyl), np.array(straddle)


def hole_case():
    """centres that are zero, NaN, +inf, negative: HOLE; the corner beside each of them has ONE such neighbour: OK (8 valid samples)"""
    depth = np.full((48, 64), 1.0, np.float32)
    bad = [0.0, np.nan, np.inf, -1.0]
    xyl, want = [], []
    for k, v in enumerate(bad):
        depth[10, 10 + 10 * k] = v
        xyl += [(10 + 10 * k, 10, 0), (11 + 10 * k, 10, 0)]
        want += [dr.HOLE, dr.OK]
    return case(depth, xyl, want)


def few_case(min_valid):
    """four of the eight neighbours zeroed: five valid samples"""
    depth = np.full((48, 64), 1.0, np.float32)
    for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        depth[20 + dy, 20 + dx] = 0.0
    return case(depth, [(20, 20, 0)], [dr.FEW if min_valid > 5 else dr.OK], min_valid=min_valid)


def border_case():
    """16 x 12 with level-2 corners (stride 4): windows that leave the image keep 4 or 6 samples"""
    depth = np.full((12, 16), 0.8, np.float32)
    xyl = [(0, 0, 2), (1, 1, 2), (3, 2, 2), (3, 1, 2), (2, 2, 2), (0, 1, 2), (4, 1, 2), (1, 3, 2)]
    want = [dr.FEW, dr.OK, dr.FEW, dr.OK, dr.OK, dr.OK, dr.OUTSIDE, dr.OUTSIDE]
    return case(depth, xyl, want)


def range_case():
    """values outside min_depth / max_depth are not valid: as a centre HOLE, as neighbours they do not count (and do not make an edge)"""
    depth = np.full((48, 64), 1.0, np.float32)
    depth[10, 10] = 0.03      # below the default min_depth
    depth[10, 30] = 4.0       # above max_depth 3
    depth[29:32, 9] = 9.0     # three neighbours of (10, 30) beyond max_depth: 6 valid, no edge
    depth[29:32, 39] = 0.04   # three neighbours of (40, 30) below min_depth
    depth[30, 51] = 2.9       # a neighbour of (50, 30) inside the limits: an edge
    xyl = [(10, 10, 0), (30, 10, 0), (10, 30, 0), (40, 30, 0), (50, 30, 0), (11, 10, 0)]
    want = [dr.HOLE, dr.HOLE, dr.OK, dr.OK, dr.EDGE, dr.OK]
    return case(depth, xyl, want, max_depth=3.0)


def designed_cases():
    """name -> case, the small ones"""
    if "designed" not in _made:
        out = {"plane": plane_case(), "step1": step_case(0.01)[0], "step20": step_case(0.20)[0], "holes": hole_case(), "few6": few_case(6),
               "few5": few_case(5), "border": border_case(), "range": range_case()}
        _made["designed"] = out
    return _made["designed"]


def filtered_corners(orc, img):
    corners = orc.detect_pyramid(img)
    return corners[orc.filter_corners(img, corners)]


SHELF_FRAMES = ((0, 0), (0, 20), (0, 39), (1, 0), (1, 20), (1, 39))   # (tracker, frame)


def shelf_case(orc, i, k):
    """frame k of tracker i's `shelf` trajectory, no lens: the oracle's filtered corners and the renderer's depth"""
    key = ("shelf", i, k)
    if key not in _made:
        ss = sc.scene_synth()
        T = trajectory_pose(orc, k, sc.tracker_twist(i))
        img, depth, _ = ss.render(ss.scene(T, preset="shelf", seed=sc.SEED + i, frame_id=k))
        _made[key] = case(depth, filtered_corners(orc, img))
    return _made[key]


def nearest_hit_depth(scene, xn, yn):
    """camera-frame z of the nearest surface the ray (xn, yn, 1) of the scene's camera hits, inf if none"""
    R = np.array(scene.R[:]).reshape(3, 3)
    t = np.array(scene.t[:])
    C, d = -R.T @ t, R.T @ np.array([xn, yn, 1.0])
    best = np.inf
    for f in sc.surfaces_of(scene):
        n = np.array(f.plane[:3])
        den = float(n @ d)
        if abs(den) < 1e-12:
            continue
        s = (f.plane[3] - float(n @ C)) / den
        if s <= 0 or s >= best:
            continue
        foot = C + s * d - np.array(f.origin[:])
        a, b = float(foot @ np.array(f.e1[:])), float(foot @ np.array(f.e2[:]))
        if (f.half_u > 0 and abs(a) > f.half_u) or (f.half_v > 0 and abs(b) > f.half_v):
            continue
        best = s
    return best


def lens_case(orc):
    """`shelf` through the lens of config_tum_f2.cfg: the raw image and its depth from the host renderer, corners detected on the undistorted
    image as a tracker sees it -> (case, scene)"""
    if "lens" not in _made:
        ss = sc.scene_synth()
        scene = ss.scene(trajectory_pose(orc, 0), cam=TUM2_CAM, preset="shelf", seed=sc.SEED, frame_id=0, dist=TUM2_DIST)
        raw, depth, _ = ss.render(scene)
        und = orc.undistort(raw, TUM2_CAM, TUM2_DIST)
        _made["lens"] = (case(depth, filtered_corners(orc, und), cam=TUM2_CAM, dist=TUM2_DIST), scene)
    return _made["lens"]


def restate(c):
    return dr.depth_seed(c["depth"], c["xyl"], c["cam"], c["dist"], c["scale"], **c["rule"])
