"""Designed inputs for stereo rectification (tests/rectify_restatement.py), shared by the CPU test of the restatement and the GPU tests of
the device path: calibrated rigs, raw test images, and the maps' references, computed once per process and read-only.

A rig is dict(K1, D1, K2, D2, R, T, w, h).  Test infrastructure only."""
import math

import numpy as np

import rectify_restatement as rr
from oraclelib import EUROC_CAM, EUROC_DIST, TUM_CAM, TUM_DIST

NO_LENS = np.zeros(5)
TUM_TURN = (0.009, -0.017, 0.005)       # the right camera's turn against the left, a rotation vector in radians

_made = {}


def ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def rot(w):
    return np.array(rr.rotation_of([float(c) for c in w]))


def rig(K1, D1, K2, D2, R, T, w, h):
    return dict(K1=ro(np.asarray(K1, np.float64)), D1=ro(np.asarray(D1, np.float64)), K2=ro(np.asarray(K2, np.float64)),
                D2=ro(np.asarray(D2, np.float64)), R=ro(np.asarray(R, np.float64)), T=ro(np.asarray(T, np.float64)), w=w, h=h)


def rigs():
    """euroc: an EuRoC-like rig at 752 x 480 (config_euroc.cfg's left camera; the right camera's figures are made up in the data set's
    manner); tum: config_tum_f1.cfg's lens on both cameras, the right one turned by TUM_TURN; ideal: no lens, R = I, T = (-B, 0, 0);
    roll5: t_x dominant and a 5 degree roll between the cameras"""
    if "rigs" not in _made:
        k2 = (457.587, 456.134, 379.999, 255.238)
        d2 = (-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0)
        _made["rigs"] = {
            "euroc": rig(EUROC_CAM, EUROC_DIST, k2, d2, rot((0.0023, -0.0128, 0.0070)), (-0.1100, 0.0004, -0.0009), 752, 480),
            "tum": rig(TUM_CAM, TUM_DIST, TUM_CAM, TUM_DIST, rot(TUM_TURN), (-0.11, 0.002, -0.001), 640, 480),
            "ideal": rig(TUM_CAM, NO_LENS, TUM_CAM, NO_LENS, np.eye(3), (-0.11, 0.0, 0.0), 640, 480),
            "roll5": rig(TUM_CAM, EUROC_DIST, TUM_CAM, EUROC_DIST, rot((0.0, 0.0, math.radians(5.0))), (-0.12, 0.01, 0.005), 640, 480),
        }
    return _made["rigs"]


def plan_of(g, override=None, w=None, h=None):
    return rr.plan(g["K1"], g["D1"], g["K2"], g["D2"], g["R"], g["T"], w or g["w"], h or g["h"], override)


def planned(name):
    """the restatement's plan of a named rig, once"""
    key = ("plan", name)
    if key not in _made:
        _made[key] = plan_of(rigs()[name])
    return _made[key]


def sides(g, p):
    """the two cameras of a planned rig as (K, D, R_i)"""
    return (g["K1"], g["D1"], p["R1"]), (g["K2"], g["D2"], p["R2"])


def rolled(deg, w, h, K=TUM_CAM, D=TUM_DIST, zoom=1.0):
    """one camera rectified by a roll of `deg` degrees about its axis behind the lens D: K scaled to the size w x h, the rectified camera
    the raw K without the lens, times `zoom` (below 1: the rectified image sees past the raw one, pixels without a source)"""
    s = w / 640.0
    raw = np.array([K[0] * s, K[1] * s, (w - 1) / 2.0 + 0.3, (h - 1) / 2.0 - 0.2])
    rect = np.array([raw[0] * zoom, raw[0] * zoom, (w - 1) / 2.0, (h - 1) / 2.0])
    return dict(K=ro(raw), D=ro(np.asarray(D, np.float64)), R=ro(rot((0.0, 0.0, math.radians(deg)))), rect=ro(rect), w=w, h=h)


def raw_image(w, h, seed, stride=None):
    """a smooth texture with noise on top, u8 [h][stride or w]: bilinear weights and single source pixels both show"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:(stride or w)].astype(np.float64)
    t = 110 + 60 * np.sin(0.11 * xx + 0.07 * yy + rng.uniform(0, 6)) + 40 * np.sin(0.31 * xx - 0.23 * yy + rng.uniform(0, 6))
    return ro(np.clip(t + rng.integers(-30, 31, t.shape), 0, 255).astype(np.uint8))


# ---- `shelf` seen by the tum rig: raw pairs through both lenses, and the ideal pair of the rectified camera rendered directly
def R_to_quat(R):
    """a rotation matrix as qw qx qy qz (turns well below 180 degrees: qw is the largest component)"""
    R = np.asarray(R, np.float64)
    qw = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])


def compose(R, t, T_cw):
    """the pose (R, t) behind the world -> camera pose T_cw = (q, t): X -> R (R_cw X + t_cw) + t"""
    from oraclelib import quat_to_R
    R_cw, t_cw = quat_to_R(np.asarray(T_cw[:4])), np.asarray(T_cw[4:7], np.float64)
    return np.concatenate([R_to_quat(np.asarray(R) @ R_cw), np.asarray(R) @ t_cw + np.asarray(t, np.float64)])


def rig_views(T_cw, name="tum"):
    """the four views of a named rig whose raw left camera stands at T_cw: dict(raw_left, raw_right, ideal_left, ideal_right), each
    (pose, cam, dist or None) — the ideal pair is the rectified camera at R1 T_cw and the camera a baseline to its right, no lens"""
    g, p = rigs()[name], planned(name)
    ideal = compose(p["R1"], np.zeros(3), T_cw)
    right = ideal.copy()
    right[4] -= p["baseline"]
    rect = np.array(p["rect"])
    return dict(raw_left=(np.asarray(T_cw, np.float64), g["K1"], g["D1"]), raw_right=(compose(g["R"], g["T"], T_cw), g["K2"], g["D2"]),
                ideal_left=(ideal, rect, None), ideal_right=(right, rect, None))


def shelf_rig_pair(orc, k, i=0, name="tum"):
    """frame k of tracker i's `shelf` trajectory seen by the rig, host-rendered: dict(raw_left, raw_right, ideal_left, ideal_right images,
    depth = the ideal left view's true depth)"""
    import scene_cases as sc
    from oraclelib import trajectory_pose
    key = ("shelf_rig", name, i, k)
    if key not in _made:
        ss = sc.scene_synth()
        g = rigs()[name]
        out = {}
        for view, (T, cam, dist) in rig_views(trajectory_pose(orc, k, sc.tracker_twist(i)), name).items():
            scene = ss.scene(T, cam=cam, preset="shelf", seed=sc.SEED + i, frame_id=k, dist=dist)
            if view == "ideal_left":
                out[view], depth, _ = ss.render(scene, g["w"], g["h"])
                out["depth"] = ro(depth)
            else:
                out[view] = ss.render(scene, g["w"], g["h"], truth=False)
            out[view] = ro(out[view])
        _made[key] = out
    return _made[key]


def disparity_figures(status, disparity, xyl, depth, f, baseline):
    """the OK share of the corners and the median |disparity - f B / true depth| of the OK ones, in pixels"""
    xyl = np.asarray(xyl, np.int64)
    s = 1 << xyl[:, 2]
    ok = np.asarray(status) == 0
    truth = f * baseline / depth[xyl[:, 1] * s, xyl[:, 0] * s].astype(np.float64)
    return float(ok.mean()), float(np.median(np.abs(np.asarray(disparity)[ok] - truth[ok])))


COMPOSITION_FRAMES = (0, 26)


# the sizes where the launches change form: W < 8 (tap by tap), a width that is no multiple of 4, more than one tile a side, the
# camera's size, the wide map
SIZES = ((6, 5), (38, 22), (130, 70), (640, 480), (2048, 10))
ROLLS = (0.5, 6.0)


def turned_away_case(w=130, h=70, deg=80.0):
    """a camera rectified by a turn of `deg` degrees about its y axis: the rays of the pixels on one side do not point forward in the raw
    camera's frame (w <= 0) and have no source, whatever x / w would say; once"""
    key = ("turned", w, h, deg)
    if key not in _made:
        c = rolled(0.0, w, h)
        c["R"] = ro(rot((0.0, math.radians(deg), 0.0)))
        iu, iv = rr.map_fixed(c["K"], c["D"], c["R"], c["rect"], w, h)
        c.update(iu=ro(iu), iv=ro(iv), no_source=rr.no_source(iu, iv, w, h))
        _made[key] = c
    return _made[key]


def byte_case(w, h, deg, zoom=1.0):
    """a rolled camera of the size, its map (iu, iv) and the count of pixels without a source, once"""
    key = ("bytes", w, h, deg, zoom)
    if key not in _made:
        c = rolled(deg, w, h, zoom=zoom)
        iu, iv = rr.map_fixed(c["K"], c["D"], c["R"], c["rect"], w, h)
        c.update(iu=ro(iu), iv=ro(iv), no_source=rr.no_source(iu, iv, w, h))
        _made[key] = c
    return _made[key]


# The rectified pair is held to the ideal pair's figures loosened by a margin measured WITHOUT the device, with the host renderer and the
# two restatements (test_rectify_restatement_cpu.py prints and checks them): the OK share of frame 26 falls 0.0144 short of the ideal
# pair's (0.8588 against 0.8731; frame 0 gains 0.0070) and the median disparity error is lower on both frames (0.0621 / 0.0586 px against
# 0.0680 / 0.0638 px), a deficit of 0.  Twice the deficit is allowed, because interpolation blurs: 0.0288 of OK share, and nothing for the
# median — the rectified pair's median may not exceed the ideal pair's.
SHARE_MARGIN = 2 * 0.0144
MEDIAN_MARGIN_PX = 2 * 0.0


def composition_reference(orc, k):
    """frame k of COMPOSITION_FRAMES without the device: the two restatements on the host-rendered raw pair, and the matcher's
    restatement on the ideal pair -> dict(rectified = (share, median), ideal = (share, median), left, right = the rectified images)"""
    import stereo_cases as stc
    import stereo_restatement as sr
    key = ("composition", k)
    if key not in _made:
        g, p, v = rigs()["tum"], planned("tum"), shelf_rig_pair(orc, k)
        rect = np.array(p["rect"])
        left = rr.rectify(np.array(v["raw_left"]), g["K1"], g["D1"], p["R1"], rect)
        right = rr.rectify(np.array(v["raw_right"]), g["K2"], g["D2"], p["R2"], rect)
        out = dict(left=ro(left), right=ro(right))
        for name, (l, r) in (("rectified", (left, right)), ("ideal", (np.array(v["ideal_left"]), np.array(v["ideal_right"])))):
            xyl = stc.filtered_corners(orc, l)
            res = sr.stereo_depth(l, r, xyl, rect, p["baseline"])
            out[name] = disparity_figures(res["status"], res["disparity"], xyl, v["depth"], rect[0], p["baseline"])
        _made[key] = out
    return _made[key]


def assert_composition(rectified, ideal):
    assert rectified[0] >= ideal[0] - SHARE_MARGIN, (rectified, ideal)
    assert rectified[1] <= ideal[1] + MEDIAN_MARGIN_PX, (rectified, ideal)
